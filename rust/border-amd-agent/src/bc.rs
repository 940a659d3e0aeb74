//! `Bc` (`border-candle-agent/src/bc/base.rs`) over the C ABI: behaviour cloning.  The policy is a plain `Mlp` with an output
//! activation; there is no critic, no target and no noise.
use crate::{
    bytes::{ActFromRows, ObsRows, RowBatch},
    config::{BcActionType, BcConfig},
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

/// BC agent on one MI355X (`Bc<E, P, R>`).  Observation rows are `obs_dim` f32; data action rows `act_dim` f32.
pub struct AmdBc<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    pub(crate) a: AgentHandle,
    act_dim: usize,
    action_type: BcActionType,
    phantom: PhantomData<(E, O, A)>,
}

impl<E, O, A> AmdBc<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    /// Parameter model id of `bdr_agent_{get,set}_params` for BC: the policy.
    pub const POLICY: i32 = 0;

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

    pub fn sync(&mut self) -> Result<()> {
        self.a.sync()
    }

    /// `policy_model.safetensors` instead of the reference's `policy_model.pt` (both hold safetensors).
    pub fn set_checkpoint_format(&mut self, safetensors: bool) -> Result<()> {
        self.a.set_checkpoint_format(safetensors)
    }
}

fn as_f32(bytes: &[u8]) -> &[f32] {
    debug_assert_eq!(bytes.len() % 4, 0);
    debug_assert_eq!(bytes.as_ptr() as usize % 4, 0);
    // SAFETY: ObsRows of a BC environment hands out the bytes of an f32 buffer (checked above in debug builds).
    unsafe { std::slice::from_raw_parts(bytes.as_ptr() as *const f32, bytes.len() / 4) }
}

impl<E, O, A> Policy<E> for AmdBc<E, O, A>
where
    E: Env,
    E::Obs: ObsRows,
    E::Act: ActFromRows<f32> + ActFromRows<i64>,
    O: RowBatch,
    A: RowBatch,
{
    /// bc/base.rs:49-59: Continuous returns the network output, Discrete the argmax over the last dimension as i64.
    fn sample(&mut self, obs: &E::Obs) -> E::Act {
        let n = obs.n_procs();
        let x = as_f32(obs.as_bytes()).as_ptr();
        match self.action_type {
            BcActionType::Continuous => {
                let mut act = vec![0f32; n * self.act_dim];
                expect(unsafe { ffi::bdr_bc_sample(self.a.h, n as u64, x, act.as_mut_ptr(), std::ptr::null_mut()) }, "Policy::sample");
                <E::Act as ActFromRows<f32>>::from_rows(act, n)
            }
            BcActionType::Discrete => {
                let mut idx = vec![0i64; n];
                expect(unsafe { ffi::bdr_bc_sample(self.a.h, n as u64, x, std::ptr::null_mut(), idx.as_mut_ptr()) }, "Policy::sample");
                <E::Act as ActFromRows<i64>>::from_rows(idx, n)
            }
        }
    }
}

impl<E, O, A> Configurable for AmdBc<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    type Config = BcConfig;

    /// bc/base.rs:126-136.
    fn build(config: Self::Config) -> Self {
        let c = config.to_c().expect("BcConfig");
        let mut h = std::ptr::null_mut();
        expect(unsafe { ffi::bdr_bc_create(&c, &mut h) }, "Bc::build");
        Self { a: AgentHandle::new(h), act_dim: c.act_dim as usize, action_type: config.action_type, phantom: PhantomData }
    }
}

impl<E, O, A> Agent<E, AmdReplayBuffer<O, A>> for AmdBc<E, O, A>
where
    E: Env + 'static,
    E::Obs: ObsRows,
    E::Act: ActFromRows<f32> + ActFromRows<i64>,
    O: RowBatch + 'static,
    A: RowBatch + 'static,
{
    /// bc/base.rs:104-106: nothing to switch.
    fn train(&mut self) {
        self.a.set_train(true);
    }

    fn eval(&mut self) {
        self.a.set_train(false);
    }

    /// bc/base.rs:110-112: always false.
    fn is_train(&self) -> bool {
        false
    }

    /// bc/base.rs:167-198 (`opt_`): one batch, `mse(policy(obs), act)`, one optimizer step.  A Discrete agent has no update (the
    /// reference panics, :174; the library reports `BDR_ERR_INVALID`).
    fn opt(&mut self, buffer: &mut AmdReplayBuffer<O, A>) {
        self.a.opt(buffer.h);
    }

    /// The record's one key: `loss`.
    fn opt_with_record(&mut self, buffer: &mut AmdReplayBuffer<O, A>) -> Record {
        self.a.opt_with_record(buffer.h)
    }

    /// bc/base.rs:138-145: `policy_model.pt`.
    fn save_params(&self, path: &Path) -> Result<Vec<PathBuf>> {
        self.a.save_params_candle(path, &["policy_model".to_string()])
    }

    /// bc/base.rs:147-153.
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

impl<E, O, A> SyncModel for AmdBc<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    type ModelInfo = Vec<f32>;

    /// The policy's parameters (model 0).
    fn model_info(&self) -> (usize, Self::ModelInfo) {
        (self.a.n_opts(), self.a.get_params(Self::POLICY))
    }

    fn sync_model(&mut self, model_info: &Self::ModelInfo) {
        self.a.set_params(Self::POLICY, model_info);
    }
}
