//! `Dqn` of border-candle-agent (`border-candle-agent/src/dqn/base.rs`) with an `Mlp` Q-network over the C ABI: online RL, the agent
//! of `examples/gym/dqn_cartpole`.  Not [`crate::dqn::AmdDqn`], which mirrors border-tch-agent's DQN: this one draws its exploration
//! from the reference's `SmallRng::seed_from_u64(42)` stream (`WeightedIndex` softmax, `gen::<u64>() % n` random actions, one
//! `gen_range` in evaluation mode), steps with candle's optimizers and writes `qnet.pt` / `qnet_tgt.pt` as safetensors.
use crate::{
    bytes::{DiscreteAct, ObsRows, RowBatch},
    config::CandleDqnConfig,
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
    ffi::c_void,
    marker::PhantomData,
    path::{Path, PathBuf},
};

/// candle DQN agent on one MI355X (`Dqn<E, Q, R>` with `Q = Mlp`).  Observation rows are `obs_dim` f32, an action row is one i64.
pub struct AmdCandleDqn<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    pub(crate) a: AgentHandle,
    train: bool,
    n_actions: usize,
    phantom: PhantomData<(E, O, A)>,
}

impl<E, O, A> AmdCandleDqn<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    /// Parameter model ids of `bdr_agent_{get,set}_params` for the candle DQN.
    pub const QNET: i32 = 0;
    pub const QNET_TGT: i32 = 1;
    pub const EXP_AVG: i32 = 2;
    pub const EXP_AVG_SQ: i32 = 3;
    pub const GRAD: i32 = 4;

    pub fn handle(&self) -> *mut ffi::bdr_agent {
        self.a.h
    }

    pub fn n_opts(&self) -> usize {
        self.a.n_opts()
    }

    pub fn n_actions(&self) -> usize {
        self.n_actions
    }

    /// Width of one action row in elements ([`crate::evaluator::SampleRaw`]): one i64 index.
    pub fn act_dim(&self) -> usize {
        1
    }

    pub fn sync(&mut self) -> Result<()> {
        self.a.sync()
    }

    /// `<stem>.safetensors` instead of the reference's `<stem>.pt` (both hold safetensors).
    pub fn set_checkpoint_format(&mut self, safetensors: bool) -> Result<()> {
        self.a.set_checkpoint_format(safetensors)
    }

    /// Q(obs) and the first-maximum actions for `n_procs` observation rows (`qnet.forward`, dqn/base.rs:203).
    pub fn qvalues(&mut self, obs: &E::Obs) -> (Vec<f32>, Vec<i64>)
    where
        E::Obs: ObsRows,
    {
        let n = obs.n_procs();
        let mut q = vec![0f32; n * self.n_actions];
        let mut best = vec![0i64; n];
        expect(
            unsafe { ffi::bdr_agent_qvalues(self.a.h, n as u64, obs.as_bytes().as_ptr() as *const c_void, q.as_mut_ptr(), best.as_mut_ptr()) },
            "bdr_agent_qvalues",
        );
        (q, best)
    }
}

impl<E, O, A> Policy<E> for AmdCandleDqn<E, O, A>
where
    E: Env,
    E::Obs: ObsRows,
    E::Act: DiscreteAct,
    O: RowBatch,
    A: RowBatch,
{
    /// dqn/base.rs:202-230 in one call: forward on the GPU, then `DqnConfig::explorer` in training mode (softmax through
    /// `WeightedIndex`, or epsilon-greedy with one f32 coin per call) / argmax with 1 % random actions in evaluation mode.  In
    /// evaluation mode the reference returns ONE action for the call; here it is written to every row.
    fn sample(&mut self, obs: &E::Obs) -> E::Act {
        let n = obs.n_procs();
        let mut act = vec![0i64; n];
        expect(
            unsafe {
                ffi::bdr_agent_sample(self.a.h, n as u64, obs.as_bytes().as_ptr() as *const c_void, act.as_mut_ptr(), std::ptr::null_mut())
            },
            "Policy::sample",
        );
        E::Act::from_rows(act, n)
    }
}

impl<E, O, A> Configurable for AmdCandleDqn<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    type Config = CandleDqnConfig;

    /// dqn/base.rs:244-276: both networks, `track(qnet_tgt, qnet, 1.0)`, the explorer and the SmallRng.  Panics where the reference
    /// panics ("No device is given for DQN agent").
    fn build(config: Self::Config) -> Self {
        let c = config.to_c().expect("CandleDqnConfig");
        let mut h = std::ptr::null_mut();
        expect(unsafe { ffi::bdr_candle_dqn_create(&c, &mut h) }, "Dqn::build");
        Self { a: AgentHandle::new(h), train: config.train, n_actions: c.n_actions as usize, phantom: PhantomData }
    }
}

impl<E, O, A> AmdCandleDqn<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    /// `Dqn<E, AtariCnn, R>::build` of border-candle-agent (the network of `examples/atari/dqn_atari`): conv1-conv3, l1, l2 on u8
    /// frame stacks.  Everything else - `opt`, `sample`, the records, `qnet.pt` / `qnet_tgt.pt` - is this type's, unchanged.
    pub fn build_atari_cnn(config: crate::config::CandleDqnAtariCnnConfig) -> Self {
        let c = config.to_c().expect("CandleDqnAtariCnnConfig");
        let mut h = std::ptr::null_mut();
        expect(unsafe { ffi::bdr_candle_dqn_cnn_create(&c, &mut h) }, "Dqn::build");
        Self { a: AgentHandle::new(h), train: config.dqn.train, n_actions: c.out_dim as usize, phantom: PhantomData }
    }
}

impl<E, O, A> Agent<E, AmdReplayBuffer<O, A>> for AmdCandleDqn<E, O, A>
where
    E: Env + 'static,
    E::Obs: ObsRows,
    E::Act: DiscreteAct,
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

    /// dqn/base.rs:172-190 (`opt_`): `n_updates_per_opt` critic updates, then the soft update when the counter of opts reaches
    /// `soft_update_interval`.  A prioritized buffer is an error: the reference panics on a weighted batch (:135-137).
    fn opt(&mut self, buffer: &mut AmdReplayBuffer<O, A>) {
        self.a.opt(buffer.h);
    }

    /// dqn/base.rs:307-331: the last update's `loss` (and, with `record_verbose_level >= 2`, the four means and the statistics of
    /// every qnet variable), then `ratio_best_act`, which resets both counters.
    fn opt_with_record(&mut self, buffer: &mut AmdReplayBuffer<O, A>) -> Record {
        self.a.opt_with_record(buffer.h)
    }

    /// dqn/base.rs:337-345: `qnet.pt`, `qnet_tgt.pt`.
    fn save_params(&self, path: &Path) -> Result<Vec<PathBuf>> {
        let stems: Vec<String> = ["qnet", "qnet_tgt"].iter().map(|s| s.to_string()).collect();
        self.a.save_params_candle(path, &stems)
    }

    /// dqn/base.rs:347-351.
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

impl<E, O, A> SyncModel for AmdCandleDqn<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    type ModelInfo = Vec<f32>;

    /// The reference leaves `SyncModel` unwritten for this agent (dqn/base.rs:380-392); the generic arena path ships the online
    /// Q-network (model 0).
    fn model_info(&self) -> (usize, Self::ModelInfo) {
        (self.a.n_opts(), self.a.get_params(Self::QNET))
    }

    fn sync_model(&mut self, model_info: &Self::ModelInfo) {
        self.a.set_params(Self::QNET, model_info);
    }
}
