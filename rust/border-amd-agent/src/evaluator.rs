//! The Evaluator of the Trainer loops and `Trainer::post_process` over the C ABI (`csrc/trainer.hip`).
//!
//! * [`AmdEvaluator`] - `DefaultEvaluator` (`border-core/src/evaluator/default_evaluator.rs:64-88`; `MinariEvaluator`,
//!   `border-minari/src/evaluator.rs:25-62`, is the same loop) behind `bdr_evaluate`: `n_episodes` episodes from
//!   `Env::reset_with_index(ix)`, `Policy::sample` -> `Env::step` until the step is done, one f32 sum of the rewards in call order.
//!   The environment is reached through two `extern "C"` trampolines; rows that are float64 or need an [`AmdObsNorm`] reach the
//!   agent through `bdr_agent_sample_raw`, rounded and normalised on the device.
//! * [`TrainerPost`] - `Trainer::post_process` (`trainer.rs:231-264`) for `bdr_trainer_train_post` /
//!   `bdr_trainer_train_offline_post`: evaluate every `eval_interval` opt steps between `eval()` and `train()`, keep the best
//!   model under `model_dir/best`, save every `save_interval` opt steps under `model_dir/<opt_steps>`; 0 means never.
//! * [`SampleRaw`] - `sample_raw` / `set_act_path` on [`AmdIql`], [`AmdAwac`], [`AmdCandleSac`], [`AmdBc`] and [`AmdCandleDqn`].
use crate::{
    awac::AmdAwac,
    bc::AmdBc,
    candle_dqn::AmdCandleDqn,
    bytes::{ActFromRows, ObsRows, RowBatch},
    candle_sac::AmdCandleSac,
    dataset::{AmdObsNorm, ObsElem},
    error::check,
    ffi,
    iql::AmdIql,
};
use anyhow::Result;
use border_core::Env;
use std::{
    ffi::CString,
    os::raw::c_void,
    path::Path,
};

/// How `Policy::sample` of a dense-agent agent runs (`bdr_agent_set_act_path`); both forms produce the same bits.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum ActPath {
    Default,
    /// pack, one launch per layer, the sample kernel
    Layers,
    /// `k_dense_act`: one launch from the raw rows to the action
    Fused,
}

impl ActPath {
    fn code(self) -> i32 {
        match self {
            ActPath::Default => ffi::BDR_ACT_PATH_DEFAULT,
            ActPath::Layers => ffi::BDR_ACT_PATH_LAYERS,
            ActPath::Fused => ffi::BDR_ACT_PATH_FUSED,
        }
    }
}

/// A settable hyperparameter of a BC, IQL, AWAC or candle SAC agent (`BDR_HYPER_*`): BC has `Lr` .. `WeightDecay`; the others the
/// learning rate and optimizer scalars of each of their models, `Gamma`, `CriticTau` and what their loss reads (`TauIql`, `InvLambda`,
/// `ExpAdvMax`; with `EntCoefMode::Auto` `EntCoefLr`, `TargetEntropy`).  An id the agent's kind does not have is an error.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Hyper {
    Lr,
    Beta1,
    Beta2,
    Eps,
    WeightDecay,
    LrActor,
    ActorBeta1,
    ActorBeta2,
    ActorEps,
    ActorWeightDecay,
    LrCritic,
    CriticBeta1,
    CriticBeta2,
    CriticEps,
    CriticWeightDecay,
    LrValue,
    ValueBeta1,
    ValueBeta2,
    ValueEps,
    ValueWeightDecay,
    Gamma,
    CriticTau,
    TauIql,
    InvLambda,
    ExpAdvMax,
    EntCoefLr,
    TargetEntropy,
}

impl Hyper {
    pub fn code(self) -> i32 {
        match self {
            Hyper::Lr => ffi::BDR_HYPER_LR,
            Hyper::Beta1 => ffi::BDR_HYPER_BETA1,
            Hyper::Beta2 => ffi::BDR_HYPER_BETA2,
            Hyper::Eps => ffi::BDR_HYPER_EPS,
            Hyper::WeightDecay => ffi::BDR_HYPER_WEIGHT_DECAY,
            Hyper::LrActor => ffi::BDR_HYPER_LR_ACTOR,
            Hyper::ActorBeta1 => ffi::BDR_HYPER_ACTOR_BETA1,
            Hyper::ActorBeta2 => ffi::BDR_HYPER_ACTOR_BETA2,
            Hyper::ActorEps => ffi::BDR_HYPER_ACTOR_EPS,
            Hyper::ActorWeightDecay => ffi::BDR_HYPER_ACTOR_WEIGHT_DECAY,
            Hyper::LrCritic => ffi::BDR_HYPER_LR_CRITIC,
            Hyper::CriticBeta1 => ffi::BDR_HYPER_CRITIC_BETA1,
            Hyper::CriticBeta2 => ffi::BDR_HYPER_CRITIC_BETA2,
            Hyper::CriticEps => ffi::BDR_HYPER_CRITIC_EPS,
            Hyper::CriticWeightDecay => ffi::BDR_HYPER_CRITIC_WEIGHT_DECAY,
            Hyper::LrValue => ffi::BDR_HYPER_LR_VALUE,
            Hyper::ValueBeta1 => ffi::BDR_HYPER_VALUE_BETA1,
            Hyper::ValueBeta2 => ffi::BDR_HYPER_VALUE_BETA2,
            Hyper::ValueEps => ffi::BDR_HYPER_VALUE_EPS,
            Hyper::ValueWeightDecay => ffi::BDR_HYPER_VALUE_WEIGHT_DECAY,
            Hyper::Gamma => ffi::BDR_HYPER_GAMMA,
            Hyper::CriticTau => ffi::BDR_HYPER_CRITIC_TAU,
            Hyper::TauIql => ffi::BDR_HYPER_TAU_IQL,
            Hyper::InvLambda => ffi::BDR_HYPER_INV_LAMBDA,
            Hyper::ExpAdvMax => ffi::BDR_HYPER_EXP_ADV_MAX,
            Hyper::EntCoefLr => ffi::BDR_HYPER_ENT_COEF_LR,
            Hyper::TargetEntropy => ffi::BDR_HYPER_TARGET_ENTROPY,
        }
    }
}

/// `Policy::sample` on raw environment rows (`bdr_agent_sample_raw`) and the choice of the acting path.
pub trait SampleRaw {
    fn raw_handle(&self) -> *mut ffi::bdr_agent;
    fn raw_act_dim(&self) -> usize;

    /// The value of one settable hyperparameter (`bdr_agent_hyper_get`).
    fn hyper(&self, id: Hyper) -> Result<f64> {
        let mut v = 0f64;
        check(unsafe { ffi::bdr_agent_hyper_get(self.raw_handle(), id.code(), &mut v) })?;
        Ok(v)
    }

    /// Sets it (`bdr_agent_hyper_set`): in force from the agent's next update, standalone or as a group member.  A value outside
    /// the field's range is an error and changes nothing.
    fn set_hyper(&mut self, id: Hyper, v: f64) -> Result<()> {
        check(unsafe { ffi::bdr_agent_hyper_set(self.raw_handle(), id.code(), v) })
    }

    /// `ActPath::Fused` on a network the kernel does not cover (a padded layer wider than 512) is an error with the reason.
    fn set_act_path(&mut self, path: ActPath) -> Result<()> {
        check(unsafe { ffi::bdr_agent_set_act_path(self.raw_handle(), path.code()) })
    }

    /// `n` contiguous host rows of `obs_dim` elements (f32 or f64) -> `[n][act_dim]` f32 actions.  With `norm` the rows are
    /// normalised on the device with the bits of [`AmdObsNorm::apply`].
    fn sample_raw<X: ObsElem>(&mut self, norm: Option<&AmdObsNorm>, n: usize, rows: &[X]) -> Result<Vec<f32>> {
        let mut act = vec![0f32; n * self.raw_act_dim()];
        let np = norm.map_or(std::ptr::null(), |m| m.handle() as *const ffi::bdr_obs_norm);
        check(unsafe {
            ffi::bdr_agent_sample_raw(self.raw_handle(), np, n as u64, rows.as_ptr() as *const c_void, X::DTYPE, 0, 0, act.as_mut_ptr(), std::ptr::null_mut())
        })?;
        Ok(act)
    }

    /// The same for a Discrete BC agent (`[n]` argmax indices) and the candle DQN (`[n]` explored actions).
    fn sample_raw_index<X: ObsElem>(&mut self, norm: Option<&AmdObsNorm>, n: usize, rows: &[X]) -> Result<Vec<i64>> {
        let mut idx = vec![0i64; n];
        let np = norm.map_or(std::ptr::null(), |m| m.handle() as *const ffi::bdr_obs_norm);
        check(unsafe {
            ffi::bdr_agent_sample_raw(self.raw_handle(), np, n as u64, rows.as_ptr() as *const c_void, X::DTYPE, 0, 0, std::ptr::null_mut(), idx.as_mut_ptr())
        })?;
        Ok(idx)
    }
}

macro_rules! impl_sample_raw {
    ($agent:ident) => {
        impl<E, O, A> SampleRaw for $agent<E, O, A>
        where
            E: Env,
            O: RowBatch,
            A: RowBatch,
        {
            fn raw_handle(&self) -> *mut ffi::bdr_agent {
                self.handle()
            }
            fn raw_act_dim(&self) -> usize {
                self.act_dim()
            }
        }
    };
}
impl_sample_raw!(AmdIql);
impl_sample_raw!(AmdAwac);
impl_sample_raw!(AmdCandleSac);
impl_sample_raw!(AmdBc);
impl_sample_raw!(AmdCandleDqn);   // one i64 index per row: sample_raw_index

/// What one evaluation returns (`bdr_eval_result`).
#[derive(Clone, Copy, Debug)]
pub struct EvalResult {
    pub score: f32,
    pub normalized: Option<f32>,
    pub n_steps: usize,
    pub n_episodes: usize,
}

struct EvalCtx<E: Env> {
    env: E,
    obs_row_bytes: usize,
    act_row_bytes: usize,
}

fn write_row<Ob: ObsRows>(obs: &Ob, out: *mut c_void, row_bytes: usize) -> i32 {
    let b = obs.as_bytes();
    if obs.n_procs() != 1 || b.len() != row_bytes {
        return ffi::BDR_ERR_INVALID;
    }
    // SAFETY: the compiled loop hands a buffer of obs_row_bytes bytes.
    unsafe { std::ptr::copy_nonoverlapping(b.as_ptr(), out as *mut u8, row_bytes) };
    ffi::BDR_OK
}

/// `Env::reset_with_index(ix)` (`env.rs:180`).
unsafe extern "C" fn eval_reset<E>(ctx: *mut c_void, ix: u64, obs_out: *mut c_void) -> i32
where
    E: Env,
    E::Obs: ObsRows,
{
    let ctx = &mut *(ctx as *mut EvalCtx<E>);
    let r = std::panic::catch_unwind(std::panic::AssertUnwindSafe(|| match ctx.env.reset_with_index(ix as usize) {
        Ok(obs) => write_row(&obs, obs_out, ctx.obs_row_bytes),
        Err(_) => 90,
    }));
    r.unwrap_or(90) // a panic must not unwind into C
}

/// `Env::step(&act)`: no reset.  The action row holds f32 values.
unsafe extern "C" fn eval_step<E>(ctx: *mut c_void, act: *const c_void, obs_out: *mut c_void, reward: *mut f32, is_terminated: *mut i8, is_truncated: *mut i8) -> i32
where
    E: Env,
    E::Obs: ObsRows,
    E::Act: ActFromRows<f32>,
{
    let ctx = &mut *(ctx as *mut EvalCtx<E>);
    let r = std::panic::catch_unwind(std::panic::AssertUnwindSafe(|| {
        let row = std::slice::from_raw_parts(act as *const f32, ctx.act_row_bytes / 4);
        let a = E::Act::from_rows(row.to_vec(), 1);
        let (step, _record) = ctx.env.step(&a);
        let rc = write_row(&step.obs, obs_out, ctx.obs_row_bytes);
        if rc != ffi::BDR_OK {
            return rc;
        }
        *reward = step.reward[0];
        *is_terminated = step.is_terminated[0];
        *is_truncated = step.is_truncated[0];
        ffi::BDR_OK
    }));
    r.unwrap_or(91)
}

/// `DefaultEvaluator<E>` for agents with f32 action rows (IQL, AWAC, Continuous BC, SAC).  `X` is the element type of the
/// environment's observation rows (f32, or f64 for Minari environments).
pub struct AmdEvaluator<E: Env> {
    ctx: Box<EvalCtx<E>>,
    c: ffi::bdr_evaluator,
}

impl<E> AmdEvaluator<E>
where
    E: Env,
    E::Obs: ObsRows,
    E::Act: ActFromRows<f32>,
{
    /// `obs_dim` elements of `X` per observation row, `act_dim` f32 per action row.
    pub fn new<X: ObsElem>(env: E, n_episodes: usize, obs_dim: usize, act_dim: usize) -> Self {
        let obs_row_bytes = obs_dim * std::mem::size_of::<X>();
        let act_row_bytes = act_dim * 4;
        let mut ctx = Box::new(EvalCtx { env, obs_row_bytes, act_row_bytes });
        // SAFETY: bdr_evaluator_default fills every field of the struct it is handed.
        let mut c: ffi::bdr_evaluator = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_evaluator_default(&mut c, std::ptr::null_mut()) };
        c.n_episodes = n_episodes as u64;
        c.obs_row_bytes = obs_row_bytes as u64;
        c.act_row_bytes = act_row_bytes as u64;
        c.obs_dtype = X::DTYPE;
        c.env = ffi::bdr_eval_env_vtable {
            ctx: &mut *ctx as *mut EvalCtx<E> as *mut c_void,
            reset_with_index: Some(eval_reset::<E>),
            step: Some(eval_step::<E>),
            obs_on_device: 0,
            device: 0,
        };
        Self { ctx, c }
    }

    /// The normaliser of the dataset the agent was trained on; it must outlive the evaluator.
    pub fn with_norm(mut self, norm: &AmdObsNorm) -> Self {
        self.c.norm = norm.handle() as *const ffi::bdr_obs_norm;
        self
    }

    /// `ref_min_score` / `ref_max_score` of a Minari dataset (`border-minari/src/env.rs:162-168`).
    pub fn with_ref_scores(mut self, min: f32, max: f32) -> Self {
        self.c.has_ref_scores = 1;
        self.c.ref_min_score = min;
        self.c.ref_max_score = max;
        self
    }

    pub fn env_mut(&mut self) -> &mut E {
        &mut self.ctx.env
    }

    pub(crate) fn as_ffi(&self) -> *const ffi::bdr_evaluator {
        &self.c
    }

    /// One evaluation of the agent behind `agent` in the mode it is in (`Evaluator::evaluate`; the Trainer switches the mode).
    pub fn evaluate(&mut self, agent: *mut ffi::bdr_agent) -> Result<EvalResult> {
        let mut out = ffi::bdr_eval_result::default();
        check(unsafe { ffi::bdr_evaluate(&self.c, agent as *mut c_void, &mut out) })?;
        Ok(EvalResult {
            score: out.score,
            normalized: if out.has_normalized != 0 { Some(out.normalized) } else { None },
            n_steps: out.n_steps as usize,
            n_episodes: out.n_episodes as usize,
        })
    }
}

/// `Trainer::post_process` for the `*_post` loops.  The model directory's string lives here, so the value must outlive the call.
pub struct TrainerPost {
    dir: CString,
    c: ffi::bdr_trainer_post,
}

impl TrainerPost {
    /// An interval of 0 means never.  Models are saved with `bdr_agent_save_params`, which creates the directory.
    pub fn new<E>(evaluator: Option<&AmdEvaluator<E>>, eval_interval: usize, save_interval: usize, model_dir: &Path) -> Result<Self>
    where
        E: Env,
        E::Obs: ObsRows,
        E::Act: ActFromRows<f32>,
    {
        let dir = CString::new(model_dir.to_string_lossy().as_bytes())?;
        // SAFETY: bdr_trainer_post_default fills every field.
        let mut c: ffi::bdr_trainer_post = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_trainer_post_default(&mut c) };
        c.eval_interval = eval_interval as u64;
        c.save_interval = save_interval as u64;
        c.evaluator = evaluator.map_or(std::ptr::null(), |e| e.as_ffi());
        c.model_dir = dir.as_ptr();
        Ok(Self { dir, c })
    }

    pub fn model_dir(&self) -> &std::ffi::CStr {
        &self.dir
    }

    /// For `ffi::bdr_trainer_train_post` / `ffi::bdr_trainer_train_offline_post`.
    pub fn as_ffi(&self) -> *const ffi::bdr_trainer_post {
        &self.c
    }

    /// `Trainer::train_offline` with post-processing on the library's own handles: `max_opts` opt steps of `agent` on `buffer`.
    pub fn train_offline(&self, config: &ffi::bdr_trainer_config, agent: *mut ffi::bdr_agent, buffer: *mut ffi::bdr_replay) -> Result<ffi::bdr_trainer_stats> {
        // SAFETY: bdr_trainer_ops_default fills every field.
        let mut ops: ffi::bdr_trainer_ops = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_trainer_ops_default(&mut ops, agent, buffer) };
        let mut st = ffi::bdr_trainer_stats::default();
        check(unsafe { ffi::bdr_trainer_train_offline_post(config, &ops, &self.c, None, std::ptr::null_mut(), &mut st) })?;
        Ok(st)
    }
}
