//! `Sac` of border-candle-agent (`border-candle-agent/src/sac/base.rs`) over the C ABI: online RL.  Critics = `MultiCritic` of `Mlp`
//! on `cat(obs, act)`, actor = `GaussianActor` over `Mlp2` (the reference's examples) or `Mlp3`, entropy coefficient `EntCoef`.
//! Not [`crate::sac::AmdSac`], which mirrors border-tch-agent's SAC.
use crate::{
    bytes::{FloatAct, ObsRows, RowBatch},
    config::CandleSacConfig,
    error::expect,
    ffi,
    handle::AgentHandle,
    replay::AmdReplayBuffer,
};
use anyhow::Result;
use border_async_trainer::SyncModel;
use border_core::{record::Record, Agent, Configurable, Env, Policy};
use std::{
    any::Any,
    marker::PhantomData,
    path::{Path, PathBuf},
};

/// candle SAC agent on one MI355X (`Sac<E, Q, P, R>`).  Observation rows are `obs_dim` f32, action rows `act_dim` f32.
pub struct AmdCandleSac<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    pub(crate) a: AgentHandle,
    train: bool,
    act_dim: usize,
    obs_dim: usize,
    n_critics: usize,
    phantom: PhantomData<(E, O, A)>,
}

impl<E, O, A> AmdCandleSac<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    /// Parameter model ids of `bdr_agent_{get,set}_params` for candle SAC.
    pub const ACTOR: i32 = 0;

    pub fn critic(&self, i: usize) -> i32 {
        1 + i as i32
    }

    pub fn critic_tgt(&self, i: usize) -> i32 {
        1 + (self.n_critics + i) as i32
    }

    /// `log_alpha` of the entropy coefficient (one value).
    pub fn log_alpha(&self) -> i32 {
        1 + 2 * self.n_critics as i32
    }

    pub fn handle(&self) -> *mut ffi::bdr_agent {
        self.a.h
    }

    pub fn n_opts(&self) -> usize {
        self.a.n_opts()
    }

    /// Width of one action row (`Policy::sample` on raw rows: [`crate::evaluator::SampleRaw`]).
    pub fn act_dim(&self) -> usize {
        self.act_dim
    }

    /// Width of one observation row.
    pub fn obs_dim(&self) -> usize {
        self.obs_dim
    }

    pub fn sync(&mut self) -> Result<()> {
        self.a.sync()
    }

    /// `<stem>.safetensors` instead of the reference's `<stem>.pt` (both hold safetensors).
    pub fn set_checkpoint_format(&mut self, safetensors: bool) -> Result<()> {
        self.a.set_checkpoint_format(safetensors)
    }
}

fn as_f32(bytes: &[u8]) -> &[f32] {
    debug_assert_eq!(bytes.len() % 4, 0);
    debug_assert_eq!(bytes.as_ptr() as usize % 4, 0);
    // SAFETY: ObsRows of a SAC environment hands out the bytes of an f32 buffer (checked above in debug builds).
    unsafe { std::slice::from_raw_parts(bytes.as_ptr() as *const f32, bytes.len() / 4) }
}

impl<E, O, A> Policy<E> for AmdCandleSac<E, O, A>
where
    E: Env,
    E::Obs: ObsRows,
    E::Act: FloatAct,
    O: RowBatch,
    A: RowBatch,
{
    /// util/actor.rs:226-241: training `mean + std * z`, evaluation `mean`, then clamp or `scale * tanh`; `z` from the agent's seeded
    /// device stream (the reference draws it from candle's generator).
    fn sample(&mut self, obs: &E::Obs) -> E::Act {
        let n = obs.n_procs();
        let mut act = vec![0f32; n * self.act_dim];
        expect(unsafe { ffi::bdr_candle_sac_sample(self.a.h, n as u64, as_f32(obs.as_bytes()).as_ptr(), act.as_mut_ptr()) }, "Policy::sample");
        E::Act::from_rows(act, n)
    }
}

impl<E, O, A> Configurable for AmdCandleSac<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    type Config = CandleSacConfig;

    /// sac/base.rs:183-210: the agent starts in eval mode unless `train` is set.
    fn build(config: Self::Config) -> Self {
        let c = config.to_c().expect("CandleSacConfig");
        let mut h = std::ptr::null_mut();
        expect(unsafe { ffi::bdr_candle_sac_create(&c, &mut h) }, "Sac::build");
        Self { a: AgentHandle::new(h), train: config.train, act_dim: c.act_dim as usize, obs_dim: c.obs_dim as usize, n_critics: c.n_critics as usize, phantom: PhantomData }
    }
}

impl<E, O, A> Agent<E, AmdReplayBuffer<O, A>> for AmdCandleSac<E, O, A>
where
    E: Env + 'static,
    E::Obs: ObsRows,
    E::Act: FloatAct,
    O: RowBatch + 'static,
    A: RowBatch + 'static,
{
    fn train(&mut self) {
        self.train = true;
        self.a.set_train(true);
    }

    fn eval(&mut self) {
        self.train = false;
        self.a.set_train(false);
    }

    fn is_train(&self) -> bool {
        self.train
    }

    /// sac/base.rs:124-134 (`opt_`), per update and in this order: batch; the entropy coefficient's step and the actor step through
    /// the minimum of the ONLINE critics; critic step with `next_act` from the UPDATED actor and alpha, the soft update of every target.
    fn opt(&mut self, buffer: &mut AmdReplayBuffer<O, A>) {
        self.a.opt(buffer.h);
    }

    /// `loss_critic`, `loss_actor` (averaged over `n_updates_per_opt`) and `ent_coef` (alpha after the last update), sac/base.rs:136-146.
    fn opt_with_record(&mut self, buffer: &mut AmdReplayBuffer<O, A>) -> Record {
        self.a.opt_with_record(buffer.h)
    }

    /// sac/base.rs:244-262: `actor.pt`, `critic.pt`, `critic.tgt.pt` (the ONLINE critics, util/critic.rs:272-285), `ent_coef.pt`.
    fn save_params(&self, path: &Path) -> Result<Vec<PathBuf>> {
        let stems: Vec<String> = ["actor", "critic", "critic.tgt", "ent_coef"].iter().map(|s| s.to_string()).collect();
        self.a.save_params_candle(path, &stems)
    }

    /// sac/base.rs:264-270: both critic files into the online critics; the targets stay as they are; `log_alpha`.
    fn load_params(&mut self, path: &Path) -> Result<()> {
        self.a.load_params(path)
    }

    fn as_any_ref(&self) -> &dyn Any {
        self
    }

    fn as_any_mut(&mut self) -> &mut dyn Any {
        self
    }
}

impl<E, O, A> SyncModel for AmdCandleSac<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    type ModelInfo = Vec<f32>;

    /// The reference has no `SyncModel` for this agent; actors need the policy only: the actor's parameters (model 0).
    fn model_info(&self) -> (usize, Self::ModelInfo) {
        (self.a.n_opts(), self.a.get_params(Self::ACTOR))
    }

    fn sync_model(&mut self, model_info: &Self::ModelInfo) {
        self.a.set_params(Self::ACTOR, model_info);
    }
}
