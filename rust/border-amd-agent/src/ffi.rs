//! Declarations of `include/border_amd.h`, one to one: every `#[repr(C)]` struct below has the header's fields in the header's
//! order with the header's types, every `extern "C"` function the header's arguments.  `tests/test_rust_shim_layout.py` of the
//! border_amd repository parses this file and the header and fails on any field / order / type / arity mismatch, so the two
//! cannot drift apart unnoticed (this image has no cargo: the check is textual, not a compile).
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_void};

pub const BDR_OK: i32 = 0;
pub const BDR_ERR_INVALID: i32 = 1;
pub const BDR_ERR_NO_DEVICE: i32 = 2;
pub const BDR_ERR_HIP: i32 = 3;
pub const BDR_ERR_EMPTY: i32 = 4;
pub const BDR_ERR_IO: i32 = 5;
pub const BDR_ERR_COMM: i32 = 6;

pub const BDR_RNG_STDRNG: i32 = 0;
pub const BDR_RNG_XOSHIRO256PP: i32 = 1;
pub const BDR_DTYPE_F32: i32 = 0;
pub const BDR_DTYPE_F64: i32 = 1;
pub const BDR_PER_NORMALIZE_ALL: i32 = 0;
pub const BDR_PER_NORMALIZE_BATCH: i32 = 1;
pub const BDR_NET_ATARI_CNN: i32 = 0;
pub const BDR_NET_MLP: i32 = 1;
pub const BDR_LOSS_MSE: i32 = 0;
pub const BDR_LOSS_SMOOTH_L1: i32 = 1;
pub const BDR_OPT_ADAM: i32 = 0;
pub const BDR_OPT_ADAMW: i32 = 1;
pub const BDR_IQN_PROBE_COS: i32 = 0;
pub const BDR_IQN_PROBE_PHI: i32 = 1;
pub const BDR_IQN_PROBE_PSI: i32 = 2;
pub const BDR_IQN_PROBE_DLIN: i32 = 3;
pub const BDR_IQN_PROBE_DPSI: i32 = 4;
pub const BDR_IQN_PROBE_TGT: i32 = 5;
pub const BDR_IQN_PROBE_LOSS_ROW: i32 = 6;
pub const BDR_IQN_PROBE_A1: i32 = 7;
pub const BDR_IQN_PROBE_A2: i32 = 8;
pub const BDR_IQN_PROBE_DY2: i32 = 9;
pub const BDR_IQN_PROBE_DY1: i32 = 10;
pub const BDR_IQN_PROBE_F_ACT: i32 = 16;
pub const BDR_IQN_PROBE_F_DY: i32 = 32;
pub const BDR_IQN_PROBE_PSI_ACT: i32 = 48;
pub const BDR_IQN_PROBE_PSI_DY: i32 = 64;
pub const BDR_SAC_PHASE_ACTOR: i32 = 0;
pub const BDR_SAC_PHASE_CRITIC: i32 = 1;
pub const BDR_SAC_BUF_X_O: i32 = 0;
pub const BDR_SAC_BUF_X_NO: i32 = 1;
pub const BDR_SAC_BUF_XQ_A: i32 = 2;
pub const BDR_SAC_BUF_XQ_N: i32 = 3;
pub const BDR_SAC_BUF_XQ_C: i32 = 4;
pub const BDR_SAC_BUF_Z: i32 = 5;
pub const BDR_SAC_BUF_T_ACT: i32 = 6;
pub const BDR_SAC_BUF_T_DY: i32 = 7;
pub const BDR_SAC_BUF_MEAN: i32 = 8;
pub const BDR_SAC_BUF_E: i32 = 9;
pub const BDR_SAC_BUF_A_S: i32 = 10;
pub const BDR_SAC_BUF_S_S: i32 = 11;
pub const BDR_SAC_BUF_SD_S: i32 = 12;
pub const BDR_SAC_BUF_LOGP: i32 = 13;
pub const BDR_SAC_BUF_GMEAN: i32 = 14;
pub const BDR_SAC_BUF_GE: i32 = 15;
pub const BDR_SAC_BUF_C_ACT: i32 = 16;
pub const BDR_SAC_BUF_C2_ACT: i32 = 17;
pub const BDR_SAC_BUF_C_DY: i32 = 18;
pub const BDR_SAC_BUF_DXQ: i32 = 19;
pub const BDR_SAC_BUF_TGT: i32 = 20;
pub const BDR_SAC_BUF_LROW: i32 = 21;
pub const BDR_SAC_BUF_SCAL: i32 = 22;
pub const BDR_SAC_BUF_LOG_ALPHA: i32 = 23;
pub const BDR_SAC_BUF_PI_PART: i32 = 24;
pub const BDR_SAC_BUF_Q_PART: i32 = 25;
pub const BDR_SAC_BUF_PI_GRAD: i32 = 26;
pub const BDR_SAC_BUF_Q_GRAD: i32 = 27;
pub const BDR_SAC_BUF_PI_CHUNKS: i32 = 28;
pub const BDR_SAC_BUF_Q_CHUNKS: i32 = 29;
pub const BDR_DQN_MLP_BUF_X_IN: i32 = 0;
pub const BDR_DQN_MLP_BUF_ACT: i32 = 1;
pub const BDR_DQN_MLP_BUF_DY: i32 = 2;
pub const BDR_DQN_MLP_BUF_PRED: i32 = 3;
pub const BDR_DQN_MLP_BUF_TGT: i32 = 4;
pub const BDR_DQN_MLP_BUF_LOSS_ROW: i32 = 5;
pub const BDR_DQN_MLP_BUF_TD_ABS: i32 = 6;
pub const BDR_DQN_MLP_BUF_LOSS: i32 = 7;
pub const BDR_DQN_MLP_BUF_DW_PART: i32 = 8;
pub const BDR_DQN_MLP_BUF_Q: i32 = 9;
pub const BDR_DQN_MLP_BUF_Q_TGT: i32 = 10;
pub const BDR_DQN_MLP_BUF_GRAD: i32 = 11;
pub const BDR_DQN_MLP_BUF_M: i32 = 12;
pub const BDR_DQN_MLP_BUF_V: i32 = 13;
pub const BDR_DQN_MLP_BUF_CHUNKS: i32 = 14;
pub const BDR_DQN_MLP_BUF_FORM: i32 = 15;
pub const BDR_DQN_MLP_FORM_LDS: i32 = 0;
pub const BDR_DQN_MLP_FORM_GLOBAL: i32 = 1;
pub const BDR_DQN_MLP_FORM_LAYERS_HEAD: i32 = 2;
pub const BDR_DQN_MLP_FORM_LAYERS_TD: i32 = 3;
pub const BDR_DQN_MLP_FORM_TILES: i32 = 4;
pub const BDR_ARITH_BF16X3_6: i32 = 0;
pub const BDR_ARITH_F32_EXACT: i32 = 1;
pub const BDR_ACTIVATION_NONE: i32 = 0;
pub const BDR_ACTIVATION_RELU: i32 = 1;
pub const BDR_ACTIVATION_TANH: i32 = 2;
pub const BDR_ACTIVATION_SIGMOID: i32 = 3;
pub const BDR_ACTION_LIMIT_CLAMP: i32 = 0;
pub const BDR_ACTION_LIMIT_TANH: i32 = 1;
pub const BDR_ACTOR_MLP3: i32 = 0;
pub const BDR_ACTOR_MLP2: i32 = 1;
pub const BDR_ENT_COEF_FIX: i32 = 0;
pub const BDR_ENT_COEF_AUTO: i32 = 1;
pub const BDR_BC_ACTION_DISCRETE: i32 = 0;
pub const BDR_BC_ACTION_CONTINUOUS: i32 = 1;
pub const BDR_BC_KERNEL_DEFAULT: i32 = 0;
pub const BDR_BC_KERNEL_GENERAL: i32 = 1;
pub const BDR_BC_KERNEL_FUSED: i32 = 2;
pub const BDR_BC_KERNEL_FUSED_MFMA: i32 = 3;
pub const BDR_MAX_UNITS: usize = 8;
pub const BDR_EXPLORER_SOFTMAX: i32 = 0;
pub const BDR_EXPLORER_EPS_GREEDY: i32 = 1;
pub const BDR_CKPT_TCH: i32 = 0;
pub const BDR_CKPT_SAFETENSORS: i32 = 1;
pub const BDR_GROUP_FORM_ONE_WORKGROUP: i32 = 0;
pub const BDR_GROUP_FORM_LAYERS: i32 = 1;
pub const BDR_GROUP_FORM_BC_LAYERS: i32 = 2;
pub const BDR_GROUP_FORM_IQL_LAYERS: i32 = 3;
pub const BDR_GROUP_FORM_AWAC_LAYERS: i32 = 4;
pub const BDR_GROUP_FORM_CANDLE_SAC_LAYERS: i32 = 5;
pub const BDR_GROUP_FORM_CANDLE_DQN_LAYERS: i32 = 6;
pub const BDR_IQN_CONST10: i32 = 0;
pub const BDR_IQN_CONST32: i32 = 1;
pub const BDR_IQN_UNIFORM10: i32 = 2;
pub const BDR_IQN_UNIFORM8: i32 = 3;
pub const BDR_IQN_UNIFORM32: i32 = 4;
pub const BDR_IQN_UNIFORM64: i32 = 5;
pub const BDR_IQN_MEDIAN: i32 = 6;
pub const BDR_UNIQUE_ID_BYTES: usize = 128;
pub const BDR_ASYNC_EVENT_SKIP: i32 = 0;
pub const BDR_ASYNC_EVENT_OPT: i32 = 1;
pub const BDR_ASYNC_EVENT_OPT_RECORD: i32 = 2;
pub const BDR_ASYNC_EVENT_COST: i32 = 3;
pub const BDR_ASYNC_EVENT_SYNC: i32 = 4;
pub const BDR_ASYNC_EVENT_PUSH: i32 = 5;
pub const BDR_ASYNC_EVENT_ACTOR_SYNC: i32 = 6;
pub const BDR_TRAINER_EVENT_SKIP: i32 = 0;
pub const BDR_TRAINER_EVENT_OPT: i32 = 1;
pub const BDR_TRAINER_EVENT_OPT_RECORD: i32 = 2;
pub const BDR_TRAINER_EVENT_COST: i32 = 3;
pub const BDR_TRAINER_EVENT_EVAL: i32 = 4;
pub const BDR_ACT_PATH_DEFAULT: i32 = 0;
pub const BDR_ACT_PATH_LAYERS: i32 = 1;
pub const BDR_ACT_PATH_FUSED: i32 = 2;
// BDR_HYPER_*: the settable scalar fields of a BC, IQL, AWAC or candle SAC agent (bdr_agent_hyper_get / _set)
pub const BDR_HYPER_LR: i32 = 0;
pub const BDR_HYPER_BETA1: i32 = 1;
pub const BDR_HYPER_BETA2: i32 = 2;
pub const BDR_HYPER_EPS: i32 = 3;
pub const BDR_HYPER_WEIGHT_DECAY: i32 = 4;
pub const BDR_HYPER_LR_ACTOR: i32 = 10;
pub const BDR_HYPER_ACTOR_BETA1: i32 = 11;
pub const BDR_HYPER_ACTOR_BETA2: i32 = 12;
pub const BDR_HYPER_ACTOR_EPS: i32 = 13;
pub const BDR_HYPER_ACTOR_WEIGHT_DECAY: i32 = 14;
pub const BDR_HYPER_LR_CRITIC: i32 = 20;
pub const BDR_HYPER_CRITIC_BETA1: i32 = 21;
pub const BDR_HYPER_CRITIC_BETA2: i32 = 22;
pub const BDR_HYPER_CRITIC_EPS: i32 = 23;
pub const BDR_HYPER_CRITIC_WEIGHT_DECAY: i32 = 24;
pub const BDR_HYPER_LR_VALUE: i32 = 30;
pub const BDR_HYPER_VALUE_BETA1: i32 = 31;
pub const BDR_HYPER_VALUE_BETA2: i32 = 32;
pub const BDR_HYPER_VALUE_EPS: i32 = 33;
pub const BDR_HYPER_VALUE_WEIGHT_DECAY: i32 = 34;
pub const BDR_HYPER_GAMMA: i32 = 40;
pub const BDR_HYPER_CRITIC_TAU: i32 = 41;
pub const BDR_HYPER_TAU_IQL: i32 = 42;
pub const BDR_HYPER_INV_LAMBDA: i32 = 43;
pub const BDR_HYPER_EXP_ADV_MAX: i32 = 44;
pub const BDR_HYPER_ENT_COEF_LR: i32 = 45;
pub const BDR_HYPER_TARGET_ENTROPY: i32 = 46;
/// `bdr_*_group_copy_members` flag: the destination also takes the source's settable hyperparameters
pub const BDR_COPY_HYPER: u32 = 1;

// opaque handles
/// `bdr_agent_group` (a launch grouping of Mlp DQN agents): only ever behind a pointer.
pub enum bdr_agent_group {}
/// `bdr_bc_group` (a launch grouping of BC agents): only ever behind a pointer.
pub enum bdr_bc_group {}
/// `bdr_iql_group` (a launch grouping of IQL agents): only ever behind a pointer.
pub enum bdr_iql_group {}
/// `bdr_awac_group` (a launch grouping of AWAC agents): only ever behind a pointer.
pub enum bdr_awac_group {}
/// `bdr_candle_sac_group` (a launch grouping of candle SAC agents): only ever behind a pointer.
pub enum bdr_candle_sac_group {}
/// `bdr_candle_dqn_group` (a launch grouping of candle DQN agents in the Mlp form): only ever behind a pointer.
pub enum bdr_candle_dqn_group {}
#[repr(C)]
pub struct bdr_replay {
    _private: [u8; 0],
}
#[repr(C)]
pub struct bdr_agent {
    _private: [u8; 0],
}
#[repr(C)]
pub struct bdr_comm {
    _private: [u8; 0],
}
#[repr(C)]
pub struct bdr_model_mailbox {
    _private: [u8; 0],
}
#[repr(C)]
pub struct bdr_atari_prep {
    _private: [u8; 0],
}

/// Opaque handle of an observation normaliser (`bdr_obs_norm_*`): an uninhabited type, only ever used behind a pointer.
pub enum bdr_obs_norm {}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct bdr_replay_summary {
    pub n_terminated: u64,
    pub n_truncated: u64,
    pub sum_rewards: f32,
    pub reserved: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_replay_config {
    pub capacity: u64,
    pub seed: u64,
    pub obs_row_bytes: u64,
    pub act_row_bytes: u64,
    pub device: i32,
    pub frame_stack: i32,
    pub frame_capacity: u64,
    pub index_rng: i32,
    pub reserved: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_device_batch {
    pub n: u64,
    pub obs: *const c_void,
    pub next_obs: *const c_void,
    pub act: *const c_void,
    pub reward: *const f32,
    pub is_terminated: *const i8,
    pub is_truncated: *const i8,
    pub ixs: *const u64,
    pub weight: *const f32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_per_config {
    pub alpha: f32,
    pub beta_0: f32,
    pub beta_final: f32,
    pub n_opts_final: u64,
    pub normalize: i32,
    pub reserved: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct bdr_group_info {
    pub form: i32,
    pub n_members: u32,
    pub launches_per_round: u32,
    pub reserved: u32,
    pub kernel_launches: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct bdr_per_info {
    pub n_samples: u64,
    pub n_opts: u64,
    pub beta: f32,
    pub total: f32,
    pub max_p: f32,
    pub min_p: f32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_net_config {
    pub kind: i32,
    pub n_stack: i32,
    pub in_dim: i32,
    pub n_units: i32,
    pub units: [i32; 8],
    pub out_dim: i32,
    pub activation_out: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_adamw_config {
    pub opt_kind: i32,
    pub amsgrad: i32,
    pub beta1: f64,
    pub beta2: f64,
    pub weight_decay: f64,
    pub eps: f64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_dqn_config {
    pub net: bdr_net_config,
    pub opt_kind: i32,
    pub lr: f64,
    pub beta1: f64,
    pub beta2: f64,
    pub weight_decay: f64,
    pub eps: f64,
    pub amsgrad: i32,
    pub soft_update_interval: u64,
    pub n_updates_per_opt: u64,
    pub batch_size: u64,
    pub discount_factor: f64,
    pub tau: f64,
    pub train: i32,
    pub double_dqn: i32,
    pub critic_loss: i32,
    pub has_clip_td_err: i32,
    pub clip_td_err_min: f64,
    pub clip_td_err_max: f64,
    pub record_verbose_level: i32,
    pub device: i32,
    pub param_seed: u64,
    pub arithmetic: i32,
    pub reserved: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct bdr_dqn_record {
    pub loss: f32,
    pub pred_mean: f32,
    pub reward_mean: f32,
    pub tgt_mean: f32,
    pub tgt_minus_pred_mean: f32,
    pub has_verbose: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_explorer_config {
    pub kind: i32,
    pub eps_start: f64,
    pub eps_final: f64,
    pub final_step: u64,
    pub n_calls: u64,
    pub seed: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct bdr_sample_info {
    pub eps: f64,
    pub is_random: i32,
    pub n_samples_act: u64,
    pub n_samples_best_act: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct bdr_env_vtable {
    pub ctx: *mut c_void,
    pub reset: Option<unsafe extern "C" fn(ctx: *mut c_void, obs_out: *mut c_void) -> i32>,
    pub step_with_reset: Option<
        unsafe extern "C" fn(
            ctx: *mut c_void,
            act: *const c_void,
            obs_out: *mut c_void,
            reward: *mut f32,
            is_terminated: *mut i8,
            is_truncated: *mut i8,
            init_obs_out: *mut c_void,
        ) -> i32,
    >,
    pub obs_on_device: i32,
    pub device: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct bdr_trainer_ops {
    pub agent: *mut c_void,
    pub buffer: *mut c_void,
    pub agent_set_train: Option<unsafe extern "C" fn(agent: *mut c_void, train: i32) -> i32>,
    pub agent_sample: Option<unsafe extern "C" fn(agent: *mut c_void, n_procs: u64, obs: *const c_void, act_out: *mut c_void) -> i32>,
    pub agent_opt: Option<unsafe extern "C" fn(agent: *mut c_void, buffer: *mut c_void) -> i32>,
    pub agent_opt_with_record:
        Option<unsafe extern "C" fn(agent: *mut c_void, buffer: *mut c_void, scalars: *mut f32, cap: i32, n_scalars: *mut i32) -> i32>,
    pub buffer_push: Option<
        unsafe extern "C" fn(
            buffer: *mut c_void,
            n: u64,
            obs: *const c_void,
            act: *const c_void,
            next_obs: *const c_void,
            reward: *const f32,
            is_terminated: *const i8,
            is_truncated: *const i8,
        ) -> i32,
    >,
    pub agent_sample_device:
        Option<unsafe extern "C" fn(agent: *mut c_void, n_procs: u64, obs_dev: *const c_void, row_stride: u64, act_out: *mut c_void) -> i32>,
    pub buffer_push_device: Option<
        unsafe extern "C" fn(
            buffer: *mut c_void,
            n: u64,
            obs_dev: *const c_void,
            obs_stride: u64,
            act: *const c_void,
            next_obs_dev: *const c_void,
            next_obs_stride: u64,
            reward: *const f32,
            is_terminated: *const i8,
            is_truncated: *const i8,
        ) -> i32,
    >,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_trainer_config {
    pub max_opts: u64,
    pub opt_interval: u64,
    pub warmup_period: u64,
    pub record_agent_info_interval: u64,
    pub record_compute_cost_interval: u64,
    pub obs_row_bytes: u64,
    pub act_row_bytes: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct bdr_trainer_stats {
    pub env_steps: u64,
    pub opt_steps: u64,
    pub n_records: u64,
    pub n_episodes: u64,
    pub opt_seconds: f64,
    pub sample_seconds: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct bdr_eval_env_vtable {
    pub ctx: *mut c_void,
    pub reset_with_index: Option<unsafe extern "C" fn(ctx: *mut c_void, ix: u64, obs_out: *mut c_void) -> i32>,
    pub step: Option<
        unsafe extern "C" fn(
            ctx: *mut c_void,
            act: *const c_void,
            obs_out: *mut c_void,
            reward: *mut f32,
            is_terminated: *mut i8,
            is_truncated: *mut i8,
        ) -> i32,
    >,
    pub obs_on_device: i32,
    pub device: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct bdr_evaluator {
    pub n_episodes: u64,
    pub obs_row_bytes: u64,
    pub act_row_bytes: u64,
    pub obs_dtype: i32,
    pub norm: *const bdr_obs_norm,
    pub has_ref_scores: i32,
    pub ref_min_score: f32,
    pub ref_max_score: f32,
    pub env: bdr_eval_env_vtable,
    pub agent_sample: Option<unsafe extern "C" fn(agent: *mut c_void, n_procs: u64, obs: *const c_void, act_out: *mut c_void) -> i32>,
    pub agent_sample_raw: Option<
        unsafe extern "C" fn(
            agent: *mut c_void,
            norm: *const bdr_obs_norm,
            n: u64,
            rows: *const c_void,
            dtype: i32,
            on_device: i32,
            row_stride: u64,
            act_out: *mut c_void,
        ) -> i32,
    >,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct bdr_eval_result {
    pub score: f32,
    pub has_normalized: i32,
    pub normalized: f32,
    pub n_steps: u64,
    pub n_episodes: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct bdr_trainer_post {
    pub eval_interval: u64,
    pub save_interval: u64,
    pub evaluator: *const bdr_evaluator,
    pub model_dir: *const c_char,
    pub save_params: Option<unsafe extern "C" fn(agent: *mut c_void, dir: *const c_char) -> i32>,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct bdr_group_trainer_ops {
    pub group: *mut c_void,
    pub buffers: *mut *const c_void,
    pub n_members: u32,
    pub reserved: u32,
    pub set_train: Option<unsafe extern "C" fn(group: *mut c_void, train: i32) -> i32>,
    pub sample: Option<unsafe extern "C" fn(group: *mut c_void, obs: *mut *const c_void, act_out: *mut i64) -> i32>,
    pub push: Option<
        unsafe extern "C" fn(
            group: *mut c_void,
            buffers: *mut *const c_void,
            obs: *mut *const c_void,
            act: *const i64,
            next_obs: *mut *const c_void,
            reward: *const f32,
            is_terminated: *const i8,
            is_truncated: *const i8,
        ) -> i32,
    >,
    pub opt: Option<unsafe extern "C" fn(group: *mut c_void, buffers: *mut *const c_void) -> i32>,
    pub opt_with_record: Option<
        unsafe extern "C" fn(group: *mut c_void, buffers: *mut *const c_void, scalars: *mut f32, cap_per_member: i32, n_scalars: *mut i32) -> i32,
    >,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct bdr_cgroup_trainer_ops {
    pub group: *mut c_void,
    pub buffers: *mut *const c_void,
    pub n_members: u32,
    pub reserved: u32,
    pub set_train: Option<unsafe extern "C" fn(group: *mut c_void, train: i32) -> i32>,
    pub sample: Option<unsafe extern "C" fn(group: *mut c_void, rows: *mut *const c_void, dtypes: *const i32, act_out: *mut *const f32) -> i32>,
    pub push: Option<
        unsafe extern "C" fn(
            group: *mut c_void,
            buffers: *mut *const c_void,
            rows: *mut *const c_void,
            next_rows: *mut *const c_void,
            dtypes: *const i32,
            act: *mut *const f32,
            reward: *mut *const f32,
            is_terminated: *mut *const i8,
            is_truncated: *mut *const i8,
        ) -> i32,
    >,
    pub opt: Option<unsafe extern "C" fn(group: *mut c_void, buffers: *mut *const c_void) -> i32>,
    pub opt_with_record: Option<
        unsafe extern "C" fn(group: *mut c_void, buffers: *mut *const c_void, scalars: *mut f32, cap_per_member: i32, n_scalars: *mut i32) -> i32,
    >,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct bdr_group_eval_ops {
    pub group: *mut c_void,
    pub n_members: u32,
    pub reserved: u32,
    pub sample_members:
        Option<unsafe extern "C" fn(group: *mut c_void, members: *const u32, n: u32, obs: *mut *const c_void, act_out: *mut i64) -> i32>,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct bdr_group_trainer_post {
    pub eval_interval: u64,
    pub save_interval: u64,
    pub evaluators: *const bdr_evaluator,
    pub model_dirs: *mut *const c_char,
    pub eval_ops: bdr_group_eval_ops,
    pub save_member: Option<unsafe extern "C" fn(group: *mut c_void, member: u32, dir: *const c_char) -> i32>,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct bdr_bc_group_eval_ops {
    pub group: *mut c_void,
    pub n_members: u32,
    pub reserved: u32,
    pub sample_members: Option<
        unsafe extern "C" fn(
            group: *mut c_void,
            members: *const u32,
            n_sel: u32,
            norms: *mut *const bdr_obs_norm,
            rows: *mut *const c_void,
            dtypes: *const i32,
            act_out: *mut *const f32,
        ) -> i32,
    >,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct bdr_bc_group_trainer_post {
    pub eval_interval: u64,
    pub save_interval: u64,
    pub evaluators: *const bdr_evaluator,
    pub model_dirs: *mut *const c_char,
    pub eval_ops: bdr_bc_group_eval_ops,
    pub save_member: Option<unsafe extern "C" fn(group: *mut c_void, member: u32, dir: *const c_char) -> i32>,
}

pub type bdr_trainer_observer =
    Option<unsafe extern "C" fn(ctx: *mut c_void, env_steps: u64, opt_steps: u64, event: i32, scalars: *const f32, n_scalars: i32)>;

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_async_trainer_config {
    pub max_opts: u64,
    pub warmup_period: u64,
    pub sync_interval: u64,
    pub record_agent_info_interval: u64,
    pub record_compute_cost_interval: u64,
    pub n_buffer: u64,
    pub channel_capacity: u64,
    pub warmup_sleep_ms: u64,
    pub obs_row_bytes: u64,
    pub act_row_bytes: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct bdr_learner_ops {
    pub t: bdr_trainer_ops,
    pub buffer_len: Option<unsafe extern "C" fn(buffer: *mut c_void, len: *mut u64) -> i32>,
    pub publish_model: Option<unsafe extern "C" fn(agent: *mut c_void, mailbox: *mut c_void, n_opts: u64) -> i32>,
    pub mailbox: *mut c_void,
    pub exchange: Option<unsafe extern "C" fn(ctx: *mut c_void, agent: *mut c_void, opt_steps: u64) -> i32>,
    pub exchange_ctx: *mut c_void,
    pub agree: Option<unsafe extern "C" fn(ctx: *mut c_void, local_ok: i32, all_ok: *mut i32) -> i32>,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct bdr_actor_ops {
    pub agent: *mut c_void,
    pub mailbox: *mut c_void,
    pub agent_set_train: Option<unsafe extern "C" fn(agent: *mut c_void, train: i32) -> i32>,
    pub agent_sample: Option<unsafe extern "C" fn(agent: *mut c_void, n_procs: u64, obs: *const c_void, act_out: *mut c_void) -> i32>,
    pub sync_model: Option<
        unsafe extern "C" fn(agent: *mut c_void, mailbox: *mut c_void, actor_id: u32, first: i32, n_opts_inout: *mut u64, updated: *mut i32) -> i32,
    >,
    pub agent_sample_device:
        Option<unsafe extern "C" fn(agent: *mut c_void, n_procs: u64, obs_dev: *const c_void, row_stride: u64, act_out: *mut c_void) -> i32>,
    pub env: bdr_env_vtable,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct bdr_async_stats {
    pub samples_total: u64,
    pub opt_steps: u64,
    pub n_records: u64,
    pub n_syncs: u64,
    pub n_messages: u64,
    pub duration_s: f64,
    pub samples_per_sec: f32,
    pub opt_per_sec: f32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct bdr_actor_stat {
    pub env_steps: u64,
    pub n_syncs: u64,
    pub duration_s: f64,
}

pub type bdr_async_observer =
    Option<unsafe extern "C" fn(ctx: *mut c_void, actor: u32, a: u64, b: u64, event: i32, scalars: *const f32, n: i32)>;

#[repr(C)]
#[derive(Clone, Copy)]
pub struct bdr_named_tensor {
    pub name: *const c_char,
    pub dims: *const u64,
    pub ndim: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_iqn_config {
    pub psi: bdr_net_config,
    pub feature_dim: i32,
    pub embed_dim: i32,
    pub n_f_units: i32,
    pub f_units: [i32; 8],
    pub n_actions: i32,
    pub lr: f64,
    pub soft_update_interval: u64,
    pub n_updates_per_opt: u64,
    pub batch_size: u64,
    pub discount_factor: f64,
    pub tau: f64,
    pub sample_percents_pred: i32,
    pub sample_percents_tgt: i32,
    pub sample_percents_act: i32,
    pub train: i32,
    pub device: i32,
    pub seed: u64,
    pub opt: bdr_adamw_config,
    pub arithmetic: i32,
    pub reserved: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_sac_config {
    pub obs_dim: i32,
    pub act_dim: i32,
    pub n_pi_units: i32,
    pub pi_units: [i32; 8],
    pub n_q_units: i32,
    pub q_units: [i32; 8],
    pub lr_actor: f64,
    pub lr_critic: f64,
    pub gamma: f64,
    pub tau: f64,
    pub ent_coef_auto: i32,
    pub ent_coef_alpha: f64,
    pub target_entropy: f64,
    pub ent_coef_lr: f64,
    pub epsilon: f64,
    pub min_lstd: f64,
    pub max_lstd: f64,
    pub n_updates_per_opt: u64,
    pub batch_size: u64,
    pub train: i32,
    pub critic_loss: i32,
    pub reward_scale: f64,
    pub n_critics: i32,
    pub device: i32,
    pub seed: u64,
    pub opt_actor: bdr_adamw_config,
    pub opt_critic: bdr_adamw_config,
}

/// border-candle-agent's MlpConfig (mlp/config.rs:6-11) without in/out dims
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_mlp_config {
    pub n_units: i32,
    pub units: [i32; 8],
    pub activation_out: i32,
}

/// IqlConfig (iql/config.rs:109-125) + ValueConfig, MultiCriticConfig, GaussianActorConfig
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_iql_config {
    pub obs_dim: i32,
    pub act_dim: i32,
    pub value: bdr_mlp_config,
    pub actor: bdr_mlp_config,
    pub critic: bdr_mlp_config,
    pub n_critics: i32,
    pub critic_tau: f64,
    pub lr_value: f64,
    pub lr_actor: f64,
    pub lr_critic: f64,
    pub opt_value: bdr_adamw_config,
    pub opt_actor: bdr_adamw_config,
    pub opt_critic: bdr_adamw_config,
    pub min_log_std: f64,
    pub max_log_std: f64,
    pub action_limit: i32,
    pub action_min: f64,
    pub action_max: f64,
    pub action_scale: f64,
    pub gamma: f64,
    pub tau_iql: f64,
    pub inv_lambda: f64,
    pub exp_adv_max: f64,
    pub adv_softmax: i32,
    pub critic_loss: i32,
    pub n_updates_per_opt: u64,
    pub batch_size: u64,
    pub train: i32,
    pub device: i32,
    pub seed: u64,
}

/// AwacConfig (awac/config.rs:120-141) + MultiCriticConfig, GaussianActorConfig
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_awac_config {
    pub obs_dim: i32,
    pub act_dim: i32,
    pub actor: bdr_mlp_config,
    pub critic: bdr_mlp_config,
    pub n_critics: i32,
    pub critic_tau: f64,
    pub lr_actor: f64,
    pub lr_critic: f64,
    pub opt_actor: bdr_adamw_config,
    pub opt_critic: bdr_adamw_config,
    pub min_log_std: f64,
    pub max_log_std: f64,
    pub action_limit: i32,
    pub action_min: f64,
    pub action_max: f64,
    pub action_scale: f64,
    pub gamma: f64,
    pub inv_lambda: f64,
    pub exp_adv_max: f64,
    pub adv_softmax: i32,
    pub critic_loss: i32,
    pub n_updates_per_opt: u64,
    pub batch_size: u64,
    pub train: i32,
    pub device: i32,
    pub seed: u64,
}

/// SacConfig of border-candle-agent (sac/config.rs:82-93) + MultiCriticConfig, GaussianActorConfig, EntCoefMode
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_candle_sac_config {
    pub obs_dim: i32,
    pub act_dim: i32,
    pub actor: bdr_mlp_config,
    pub critic: bdr_mlp_config,
    pub n_critics: i32,
    pub critic_tau: f64,
    pub lr_actor: f64,
    pub lr_critic: f64,
    pub opt_actor: bdr_adamw_config,
    pub opt_critic: bdr_adamw_config,
    pub min_log_std: f64,
    pub max_log_std: f64,
    pub action_limit: i32,
    pub action_min: f64,
    pub action_max: f64,
    pub action_scale: f64,
    pub gamma: f64,
    pub ent_coef_mode: i32,
    pub ent_coef_alpha: f64,
    pub target_entropy: f64,
    pub ent_coef_lr: f64,
    pub actor_kind: i32,
    pub critic_loss: i32,
    pub n_updates_per_opt: u64,
    pub batch_size: u64,
    pub train: i32,
    pub device: i32,
    pub seed: u64,
}

/// BcConfig (bc/config.rs:66-75) + BcModelConfig (bc/model.rs)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_bc_config {
    pub obs_dim: i32,
    pub act_dim: i32,
    pub policy: bdr_mlp_config,
    pub opt: bdr_adamw_config,
    pub lr: f64,
    pub batch_size: u64,
    pub action_type: i32,
    pub device: i32,
    pub record_verbose_level: i32,
    pub kernel_form: i32,
    pub head_rows: i32,
    pub reserved: i32,
    pub seed: u64,
}

/// DqnConfig of border-candle-agent (dqn/config.rs:75-102) + DqnModelConfig (dqn/model.rs) + the explorer and its SmallRng seed
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_candle_dqn_config {
    pub obs_dim: i32,
    pub n_actions: i32,
    pub qnet: bdr_mlp_config,
    pub opt: bdr_adamw_config,
    pub lr: f64,
    pub soft_update_interval: u64,
    pub n_updates_per_opt: u64,
    pub batch_size: u64,
    pub discount_factor: f64,
    pub tau: f64,
    pub train: i32,
    pub double_dqn: i32,
    pub explorer: bdr_explorer_config,
    pub has_clip_reward: i32,
    pub has_clip_td_err: i32,
    pub clip_reward: f64,
    pub clip_td_err_min: f64,
    pub clip_td_err_max: f64,
    pub critic_loss: i32,
    pub record_verbose_level: i32,
    pub device: i32,
    pub ckpt_format: i32,
    pub seed: u64,
}

/// The same agent with the candle crate's AtariCnn Q-network (atari_cnn/base.rs): AtariCnnConfig's n_stack / out_dim / skip_linear
/// in place of obs_dim / qnet, plus the library's `arithmetic` (BDR_ARITH_F32_EXACT only)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bdr_candle_dqn_cnn_config {
    pub n_stack: i32,
    pub out_dim: i32,
    pub skip_linear: i32,
    pub arithmetic: i32,
    pub opt: bdr_adamw_config,
    pub lr: f64,
    pub soft_update_interval: u64,
    pub n_updates_per_opt: u64,
    pub batch_size: u64,
    pub discount_factor: f64,
    pub tau: f64,
    pub train: i32,
    pub double_dqn: i32,
    pub explorer: bdr_explorer_config,
    pub has_clip_reward: i32,
    pub has_clip_td_err: i32,
    pub clip_reward: f64,
    pub clip_td_err_min: f64,
    pub clip_td_err_max: f64,
    pub critic_loss: i32,
    pub record_verbose_level: i32,
    pub device: i32,
    pub ckpt_format: i32,
    pub seed: u64,
}

#[link(name = "border_amd")]
extern "C" {
    pub fn bdr_last_error() -> *const c_char;
    pub fn bdr_last_error_is_deferred() -> i32;
    pub fn bdr_device_count(count: *mut i32) -> i32;
    pub fn bdr_version() -> *const c_char;

    // ---- SimpleReplayBuffer
    pub fn bdr_replay_create(cfg: *const bdr_replay_config, out: *mut *mut bdr_replay) -> i32;
    pub fn bdr_replay_destroy(r: *mut bdr_replay) -> i32;
    pub fn bdr_replay_view_create(owner: *mut bdr_replay, seed: u64, out: *mut *mut bdr_replay) -> i32;
    pub fn bdr_replay_push(
        r: *mut bdr_replay,
        n: u64,
        obs: *const c_void,
        act: *const c_void,
        next_obs: *const c_void,
        reward: *const f32,
        is_terminated: *const i8,
        is_truncated: *const i8,
    ) -> i32;
    pub fn bdr_replay_push_device(
        r: *mut bdr_replay,
        n: u64,
        obs_dev: *const c_void,
        obs_stride: u64,
        act: *const c_void,
        next_obs_dev: *const c_void,
        next_obs_stride: u64,
        reward: *const f32,
        is_terminated: *const i8,
        is_truncated: *const i8,
    ) -> i32;
    pub fn bdr_replay_push_device_frames(
        r: *mut bdr_replay,
        n: u64,
        obs_dev: *const c_void,
        obs_stride: u64,
        act: *const c_void,
        next_obs_dev: *const c_void,
        next_obs_stride: u64,
        reward: *const f32,
        is_terminated: *const i8,
        is_truncated: *const i8,
    ) -> i32;
    pub fn bdr_replay_len(r: *const bdr_replay, len: *mut u64) -> i32;
    pub fn bdr_replay_head(r: *const bdr_replay, head: *mut u64) -> i32;
    pub fn bdr_replay_frames_used(r: *const bdr_replay, allocated: *mut u64, capacity: *mut u64) -> i32;
    pub fn bdr_replay_sample_indices(r: *mut bdr_replay, n: u64, ixs_out: *mut u64) -> i32;
    pub fn bdr_replay_batch(
        r: *mut bdr_replay,
        n: u64,
        ixs_out: *mut u64,
        obs_out: *mut c_void,
        act_out: *mut c_void,
        next_obs_out: *mut c_void,
        reward_out: *mut f32,
        is_terminated_out: *mut i8,
        is_truncated_out: *mut i8,
    ) -> i32;
    pub fn bdr_replay_last_batch(r: *const bdr_replay, out: *mut bdr_device_batch) -> i32;
    pub fn bdr_replay_fill_synthetic(r: *mut bdr_replay, n: u64, seed: u64, kind: i32, n_actions: i32) -> i32;
    pub fn bdr_replay_read_rows(
        r: *mut bdr_replay,
        first: u64,
        n: u64,
        obs: *mut c_void,
        act: *mut c_void,
        next_obs: *mut c_void,
        reward: *mut f32,
        term: *mut i8,
        trunc: *mut i8,
    ) -> i32;

    // ---- prioritized replay
    pub fn bdr_per_config_default(c: *mut bdr_per_config);
    pub fn bdr_obs_norm_create(device: i32, dim: u64, out: *mut *mut bdr_obs_norm) -> i32;
    pub fn bdr_obs_norm_destroy(h: *mut bdr_obs_norm) -> i32;
    pub fn bdr_obs_norm_accumulate(h: *mut bdr_obs_norm, n_rows: u64, rows: *const c_void, dtype: i32) -> i32;
    pub fn bdr_obs_norm_finish(h: *mut bdr_obs_norm) -> i32;
    pub fn bdr_obs_norm_set(h: *mut bdr_obs_norm, mean: *const f32, std: *const f32) -> i32;
    pub fn bdr_obs_norm_get(h: *const bdr_obs_norm, mean_out: *mut f32, std_out: *mut f32, count_out: *mut u64) -> i32;
    pub fn bdr_obs_norm_apply(h: *const bdr_obs_norm, n: u64, rows: *const c_void, dtype: i32, out: *mut f32) -> i32;
    pub fn bdr_obs_norm_apply_device(
        h: *const bdr_obs_norm,
        n: u64,
        rows_dev: *const c_void,
        row_stride: u64,
        dtype: i32,
        out_dev: *mut f32,
        out_stride: u64,
    ) -> i32;
    pub fn bdr_replay_push_episode(
        r: *mut bdr_replay,
        t: u64,
        observations: *const c_void,
        obs_dtype: i32,
        act: *const c_void,
        reward: *const f32,
        is_terminated: *const i8,
        is_truncated: *const i8,
        norm: *const bdr_obs_norm,
    ) -> i32;
    pub fn bdr_replay_summarize(r: *mut bdr_replay, out: *mut bdr_replay_summary) -> i32;
    pub fn bdr_replay_enable_per(r: *mut bdr_replay, c: *const bdr_per_config) -> i32;
    pub fn bdr_replay_update_priority(r: *mut bdr_replay, n: u64, ixs: *const u64, td_errs: *const f32) -> i32;
    pub fn bdr_replay_batch_weights(r: *mut bdr_replay, n: u64, w_out: *mut f32) -> i32;
    pub fn bdr_replay_per_info(r: *mut bdr_replay, out: *mut bdr_per_info) -> i32;
    pub fn bdr_replay_per_read(r: *mut bdr_replay, what: i32, out: *mut f32, n: u64) -> i32;
    pub fn bdr_replay_per_get(r: *mut bdr_replay, s: f32, ix: *mut u64) -> i32;

    // ---- DQN and the agent surface shared by every kind
    pub fn bdr_dqn_config_default(cfg: *mut bdr_dqn_config);
    pub fn bdr_dqn_create(cfg: *const bdr_dqn_config, out: *mut *mut bdr_agent) -> i32;
    pub fn bdr_agent_destroy(a: *mut bdr_agent) -> i32;
    pub fn bdr_agent_set_train(a: *mut bdr_agent, train: i32) -> i32;
    pub fn bdr_agent_is_train(a: *const bdr_agent, out: *mut i32) -> i32;
    pub fn bdr_agent_opt(a: *mut bdr_agent, buffer: *mut bdr_replay) -> i32;
    pub fn bdr_agent_opt_with_record(a: *mut bdr_agent, buffer: *mut bdr_replay, rec: *mut bdr_dqn_record) -> i32;
    pub fn bdr_agent_opt_with_scalars(a: *mut bdr_agent, buffer: *mut bdr_replay, out: *mut f32, cap: i32, n_out: *mut i32) -> i32;
    pub fn bdr_agent_record_keys(a: *mut bdr_agent, names_out: *mut c_char, names_cap: u64, n_keys: *mut i32) -> i32;
    pub fn bdr_agent_draw_noise(a: *mut bdr_agent, n: u64, out: *mut f32) -> i32;
    pub fn bdr_dqn_update_on_batch(
        a: *mut bdr_agent,
        n: u64,
        obs: *const c_void,
        act: *const i64,
        next_obs: *const c_void,
        reward: *const f32,
        is_terminated: *const i8,
        rec: *mut bdr_dqn_record,
    ) -> i32;
    pub fn bdr_dqn_update_on_batch_weighted(
        a: *mut bdr_agent,
        n: u64,
        obs: *const c_void,
        act: *const i64,
        next_obs: *const c_void,
        reward: *const f32,
        is_terminated: *const i8,
        weight: *const f32,
        td_errs_out: *mut f32,
        rec: *mut bdr_dqn_record,
    ) -> i32;
    pub fn bdr_dqn_grads_on_batch(
        a: *mut bdr_agent,
        n: u64,
        obs: *const c_void,
        act: *const i64,
        next_obs: *const c_void,
        reward: *const f32,
        is_terminated: *const i8,
        rec: *mut bdr_dqn_record,
    ) -> i32;
    pub fn bdr_agent_apply_grads(a: *mut bdr_agent) -> i32;
    pub fn bdr_agent_qvalues(a: *mut bdr_agent, n: u64, obs: *const c_void, q_out: *mut f32, argmax_out: *mut i64) -> i32;
    pub fn bdr_explorer_config_default(e: *mut bdr_explorer_config, kind: i32);
    pub fn bdr_agent_set_explorer(a: *mut bdr_agent, e: *const bdr_explorer_config) -> i32;
    pub fn bdr_agent_get_explorer(a: *const bdr_agent, e: *mut bdr_explorer_config) -> i32;
    pub fn bdr_agent_sample(a: *mut bdr_agent, n_procs: u64, obs: *const c_void, act_out: *mut i64, info: *mut bdr_sample_info) -> i32;
    pub fn bdr_agent_sample_device(a: *mut bdr_agent, n_procs: u64, obs_dev: *const c_void, row_stride: u64, act_out: *mut i64, info: *mut bdr_sample_info) -> i32;
    pub fn bdr_agent_qvalues_device(a: *mut bdr_agent, n: u64, obs_dev: *const c_void, row_stride: u64, q_out: *mut f32, argmax_out: *mut i64) -> i32;
    pub fn bdr_agent_sync(a: *mut bdr_agent) -> i32;
    pub fn bdr_agent_n_opts(a: *const bdr_agent, n: *mut u64) -> i32;
    // Agent groups.  The header's array parameters are `T* const*` (an array of handles the callee only reads); they are spelled here
    // the way tests/test_rust_shim_layout.py canonicalises that declarator - same ABI, one pointer to an array of pointers.
    pub fn bdr_agent_group_create(agents: *mut *const bdr_agent, n: u32, out: *mut *mut bdr_agent_group) -> i32;
    pub fn bdr_agent_group_destroy(g: *mut bdr_agent_group) -> i32;
    pub fn bdr_agent_group_size(g: *const bdr_agent_group, n: *mut u32) -> i32;
    pub fn bdr_agent_group_member(g: *const bdr_agent_group, i: u32, out: *mut *mut bdr_agent) -> i32;
    pub fn bdr_agent_group_info(g: *const bdr_agent_group, out: *mut bdr_group_info) -> i32;
    pub fn bdr_agent_group_set_prioritized(g: *mut bdr_agent_group, on: i32) -> i32;
    pub fn bdr_agent_group_opt(g: *mut bdr_agent_group, buffers: *mut *const bdr_replay) -> i32;
    pub fn bdr_agent_group_opt_with_scalars(g: *mut bdr_agent_group, buffers: *mut *const bdr_replay, out: *mut f32, cap_per_member: i32, n_out: *mut i32) -> i32;
    pub fn bdr_agent_group_qvalues(g: *mut bdr_agent_group, obs: *mut *const c_void, q_out: *mut *const f32) -> i32;
    pub fn bdr_agent_group_sample(g: *mut bdr_agent_group, obs: *mut *const c_void, act_out: *mut i64, info: *mut bdr_sample_info) -> i32;
    pub fn bdr_agent_group_sample_members(
        g: *mut bdr_agent_group,
        members: *const u32,
        n: u32,
        obs: *mut *const c_void,
        act_out: *mut i64,
        info: *mut bdr_sample_info,
    ) -> i32;
    pub fn bdr_agent_group_sync(g: *mut bdr_agent_group) -> i32;
    pub fn bdr_bc_group_create(agents: *mut *const bdr_agent, n: u32, out: *mut *mut bdr_bc_group) -> i32;
    pub fn bdr_bc_group_destroy(g: *mut bdr_bc_group) -> i32;
    pub fn bdr_bc_group_size(g: *const bdr_bc_group, n: *mut u32) -> i32;
    pub fn bdr_bc_group_member(g: *const bdr_bc_group, i: u32, out: *mut *mut bdr_agent) -> i32;
    pub fn bdr_bc_group_info(g: *const bdr_bc_group, out: *mut bdr_group_info) -> i32;
    pub fn bdr_bc_group_opt(g: *mut bdr_bc_group, buffers: *mut *const bdr_replay) -> i32;
    pub fn bdr_bc_group_opt_with_scalars(g: *mut bdr_bc_group, buffers: *mut *const bdr_replay, out: *mut f32, cap_per_member: i32, n_out: *mut i32) -> i32;
    pub fn bdr_bc_group_sync(g: *mut bdr_bc_group) -> i32;
    pub fn bdr_iql_group_create(agents: *mut *const bdr_agent, n: u32, out: *mut *mut bdr_iql_group) -> i32;
    pub fn bdr_iql_group_destroy(g: *mut bdr_iql_group) -> i32;
    pub fn bdr_iql_group_size(g: *const bdr_iql_group, n: *mut u32) -> i32;
    pub fn bdr_iql_group_member(g: *const bdr_iql_group, i: u32, out: *mut *mut bdr_agent) -> i32;
    pub fn bdr_iql_group_info(g: *const bdr_iql_group, out: *mut bdr_group_info) -> i32;
    pub fn bdr_iql_group_opt(g: *mut bdr_iql_group, buffers: *mut *const bdr_replay) -> i32;
    pub fn bdr_iql_group_opt_with_scalars(g: *mut bdr_iql_group, buffers: *mut *const bdr_replay, out: *mut f32, cap_per_member: i32, n_out: *mut i32) -> i32;
    pub fn bdr_iql_group_sync(g: *mut bdr_iql_group) -> i32;
    pub fn bdr_iql_group_sample(
        g: *mut bdr_iql_group,
        norms: *mut *const bdr_obs_norm,
        n: u64,
        rows: *mut *const c_void,
        dtypes: *const i32,
        act_out: *mut *const f32,
    ) -> i32;
    pub fn bdr_iql_group_sample_members(
        g: *mut bdr_iql_group,
        members: *const u32,
        n_sel: u32,
        norms: *mut *const bdr_obs_norm,
        n: u64,
        rows: *mut *const c_void,
        dtypes: *const i32,
        act_out: *mut *const f32,
    ) -> i32;
    pub fn bdr_iql_group_eval_ops_default(ops: *mut bdr_bc_group_eval_ops, group: *mut bdr_iql_group);
    pub fn bdr_iql_group_trainer_ops_default(ops: *mut bdr_group_trainer_ops, group: *mut bdr_iql_group, buffers: *mut *const bdr_replay);
    pub fn bdr_iql_group_trainer_post_default(post: *mut bdr_bc_group_trainer_post, group: *mut bdr_iql_group);
    pub fn bdr_awac_group_create(agents: *mut *const bdr_agent, n: u32, out: *mut *mut bdr_awac_group) -> i32;
    pub fn bdr_awac_group_destroy(g: *mut bdr_awac_group) -> i32;
    pub fn bdr_awac_group_size(g: *const bdr_awac_group, n: *mut u32) -> i32;
    pub fn bdr_awac_group_member(g: *const bdr_awac_group, i: u32, out: *mut *mut bdr_agent) -> i32;
    pub fn bdr_awac_group_info(g: *const bdr_awac_group, out: *mut bdr_group_info) -> i32;
    pub fn bdr_awac_group_opt(g: *mut bdr_awac_group, buffers: *mut *const bdr_replay) -> i32;
    pub fn bdr_awac_group_opt_with_scalars(g: *mut bdr_awac_group, buffers: *mut *const bdr_replay, out: *mut f32, cap_per_member: i32, n_out: *mut i32) -> i32;
    pub fn bdr_awac_group_sync(g: *mut bdr_awac_group) -> i32;
    pub fn bdr_awac_group_sample(
        g: *mut bdr_awac_group,
        norms: *mut *const bdr_obs_norm,
        n: u64,
        rows: *mut *const c_void,
        dtypes: *const i32,
        act_out: *mut *const f32,
    ) -> i32;
    pub fn bdr_awac_group_sample_members(
        g: *mut bdr_awac_group,
        members: *const u32,
        n_sel: u32,
        norms: *mut *const bdr_obs_norm,
        n: u64,
        rows: *mut *const c_void,
        dtypes: *const i32,
        act_out: *mut *const f32,
    ) -> i32;
    pub fn bdr_awac_group_eval_ops_default(ops: *mut bdr_bc_group_eval_ops, group: *mut bdr_awac_group);
    pub fn bdr_awac_group_trainer_ops_default(ops: *mut bdr_group_trainer_ops, group: *mut bdr_awac_group, buffers: *mut *const bdr_replay);
    pub fn bdr_awac_group_trainer_post_default(post: *mut bdr_bc_group_trainer_post, group: *mut bdr_awac_group);
    pub fn bdr_awac_group_push(
        g: *mut bdr_awac_group,
        buffers: *mut *const bdr_replay,
        n: u64,
        obs: *mut *const c_void,
        next_obs: *mut *const c_void,
        obs_dtypes: *const i32,
        act: *mut *const f32,
        reward: *mut *const f32,
        is_terminated: *mut *const i8,
        is_truncated: *mut *const i8,
    ) -> i32;
    pub fn bdr_awac_group_push_max_rows(g: *mut bdr_awac_group, buffers: *mut *const bdr_replay, obs_dtypes: *const i32, n_max: *mut u64) -> i32;
    pub fn bdr_awac_group_ctrainer_ops_default(ops: *mut bdr_cgroup_trainer_ops, group: *mut bdr_awac_group, buffers: *mut *const bdr_replay);
    pub fn bdr_candle_sac_group_create(agents: *mut *const bdr_agent, n: u32, out: *mut *mut bdr_candle_sac_group) -> i32;
    pub fn bdr_candle_sac_group_destroy(g: *mut bdr_candle_sac_group) -> i32;
    pub fn bdr_candle_sac_group_size(g: *const bdr_candle_sac_group, n: *mut u32) -> i32;
    pub fn bdr_candle_sac_group_member(g: *const bdr_candle_sac_group, i: u32, out: *mut *mut bdr_agent) -> i32;
    pub fn bdr_candle_sac_group_info(g: *const bdr_candle_sac_group, out: *mut bdr_group_info) -> i32;
    pub fn bdr_candle_sac_group_opt(g: *mut bdr_candle_sac_group, buffers: *mut *const bdr_replay) -> i32;
    pub fn bdr_candle_sac_group_opt_with_scalars(g: *mut bdr_candle_sac_group, buffers: *mut *const bdr_replay, out: *mut f32, cap_per_member: i32, n_out: *mut i32) -> i32;
    pub fn bdr_candle_sac_group_sync(g: *mut bdr_candle_sac_group) -> i32;
    pub fn bdr_candle_sac_group_sample(
        g: *mut bdr_candle_sac_group,
        norms: *mut *const bdr_obs_norm,
        n: u64,
        rows: *mut *const c_void,
        dtypes: *const i32,
        act_out: *mut *const f32,
    ) -> i32;
    pub fn bdr_candle_sac_group_sample_members(
        g: *mut bdr_candle_sac_group,
        members: *const u32,
        n_sel: u32,
        norms: *mut *const bdr_obs_norm,
        n: u64,
        rows: *mut *const c_void,
        dtypes: *const i32,
        act_out: *mut *const f32,
    ) -> i32;
    pub fn bdr_candle_sac_group_eval_ops_default(ops: *mut bdr_bc_group_eval_ops, group: *mut bdr_candle_sac_group);
    pub fn bdr_candle_sac_group_trainer_ops_default(ops: *mut bdr_group_trainer_ops, group: *mut bdr_candle_sac_group, buffers: *mut *const bdr_replay);
    pub fn bdr_candle_sac_group_trainer_post_default(post: *mut bdr_bc_group_trainer_post, group: *mut bdr_candle_sac_group);
    pub fn bdr_candle_sac_group_push(
        g: *mut bdr_candle_sac_group,
        buffers: *mut *const bdr_replay,
        n: u64,
        obs: *mut *const c_void,
        next_obs: *mut *const c_void,
        obs_dtypes: *const i32,
        act: *mut *const f32,
        reward: *mut *const f32,
        is_terminated: *mut *const i8,
        is_truncated: *mut *const i8,
    ) -> i32;
    pub fn bdr_candle_sac_group_push_max_rows(g: *mut bdr_candle_sac_group, buffers: *mut *const bdr_replay, obs_dtypes: *const i32, n_max: *mut u64) -> i32;
    pub fn bdr_candle_sac_group_ctrainer_ops_default(ops: *mut bdr_cgroup_trainer_ops, group: *mut bdr_candle_sac_group, buffers: *mut *const bdr_replay);
    pub fn bdr_trainer_train_cgroup_post(
        c: *const bdr_trainer_config,
        obs_row_bytes: *const u64,
        obs_dtypes: *const i32,
        ops: *const bdr_cgroup_trainer_ops,
        envs: *const bdr_env_vtable,
        post: *const bdr_bc_group_trainer_post,
        observer: Option<
            unsafe extern "C" fn(ctx: *mut c_void, member: u32, env_steps: u64, opt_steps: u64, event: i32, scalars: *const f32, n_scalars: i32),
        >,
        observer_ctx: *mut c_void,
        out: *mut bdr_trainer_stats,
    ) -> i32;
    pub fn bdr_bc_group_sample(
        g: *mut bdr_bc_group,
        norms: *mut *const bdr_obs_norm,
        n: u64,
        rows: *mut *const c_void,
        dtypes: *const i32,
        act_out: *mut *const f32,
    ) -> i32;
    pub fn bdr_bc_group_sample_members(
        g: *mut bdr_bc_group,
        members: *const u32,
        n_sel: u32,
        norms: *mut *const bdr_obs_norm,
        n: u64,
        rows: *mut *const c_void,
        dtypes: *const i32,
        act_out: *mut *const f32,
    ) -> i32;
    pub fn bdr_bc_group_eval_ops_default(ops: *mut bdr_bc_group_eval_ops, group: *mut bdr_bc_group);
    pub fn bdr_evaluate_bc_group(evs: *const bdr_evaluator, ops: *const bdr_bc_group_eval_ops, out: *mut bdr_eval_result) -> i32;
    pub fn bdr_bc_group_trainer_ops_default(ops: *mut bdr_group_trainer_ops, group: *mut bdr_bc_group, buffers: *mut *const bdr_replay);
    pub fn bdr_bc_group_trainer_post_default(post: *mut bdr_bc_group_trainer_post, group: *mut bdr_bc_group);
    pub fn bdr_trainer_train_offline_group_post(
        c: *const bdr_trainer_config,
        ops: *const bdr_group_trainer_ops,
        post: *const bdr_bc_group_trainer_post,
        observer: Option<
            unsafe extern "C" fn(ctx: *mut c_void, member: u32, env_steps: u64, opt_steps: u64, event: i32, scalars: *const f32, n_scalars: i32),
        >,
        observer_ctx: *mut c_void,
        out: *mut bdr_trainer_stats,
    ) -> i32;
    pub fn bdr_agent_group_push(
        g: *mut bdr_agent_group,
        buffers: *mut *const bdr_replay,
        obs: *mut *const c_void,
        act: *const i64,
        next_obs: *mut *const c_void,
        reward: *const f32,
        is_terminated: *const i8,
        is_truncated: *const i8,
    ) -> i32;
    pub fn bdr_agent_param_count(a: *const bdr_agent, n: *mut u64) -> i32;
    pub fn bdr_agent_param_count_of(a: *mut bdr_agent, which: i32, n: *mut u64) -> i32;
    pub fn bdr_agent_get_params(a: *mut bdr_agent, which: i32, out: *mut f32, n: u64) -> i32;
    pub fn bdr_agent_set_params(a: *mut bdr_agent, which: i32, inp: *const f32, n: u64) -> i32;
    pub fn bdr_agent_arena_device_ptr(a: *mut bdr_agent, which: i32, ptr: *mut *mut c_void, n_floats: *mut u64) -> i32;
    pub fn bdr_agent_arena_release(a: *mut bdr_agent, which: i32) -> i32;
    pub fn bdr_agent_set_checkpoint_format(a: *mut bdr_agent, format: i32) -> i32;
    pub fn bdr_agent_save_params(a: *mut bdr_agent, dir: *const c_char) -> i32;
    pub fn bdr_agent_load_params(a: *mut bdr_agent, dir: *const c_char) -> i32;

    // ---- compiled Trainer loops
    pub fn bdr_trainer_config_default(c: *mut bdr_trainer_config);
    pub fn bdr_trainer_ops_default(ops: *mut bdr_trainer_ops, agent: *mut bdr_agent, buffer: *mut bdr_replay);
    pub fn bdr_trainer_train(
        c: *const bdr_trainer_config,
        ops: *const bdr_trainer_ops,
        env: *const bdr_env_vtable,
        observer: bdr_trainer_observer,
        observer_ctx: *mut c_void,
        out: *mut bdr_trainer_stats,
    ) -> i32;
    pub fn bdr_group_trainer_ops_default(ops: *mut bdr_group_trainer_ops, group: *mut bdr_agent_group, buffers: *mut *const bdr_replay);
    pub fn bdr_trainer_train_group(
        c: *const bdr_trainer_config,
        obs_row_bytes: *const u64,
        ops: *const bdr_group_trainer_ops,
        envs: *const bdr_env_vtable,
        observer: Option<
            unsafe extern "C" fn(ctx: *mut c_void, member: u32, env_steps: u64, opt_steps: u64, event: i32, scalars: *const f32, n_scalars: i32),
        >,
        observer_ctx: *mut c_void,
        out: *mut bdr_trainer_stats,
    ) -> i32;
    pub fn bdr_group_eval_ops_default(ops: *mut bdr_group_eval_ops, group: *mut bdr_agent_group);
    pub fn bdr_evaluate_group(evs: *const bdr_evaluator, ops: *const bdr_group_eval_ops, out: *mut bdr_eval_result) -> i32;
    pub fn bdr_group_trainer_post_default(post: *mut bdr_group_trainer_post, group: *mut bdr_agent_group);
    pub fn bdr_trainer_train_group_post(
        c: *const bdr_trainer_config,
        obs_row_bytes: *const u64,
        ops: *const bdr_group_trainer_ops,
        envs: *const bdr_env_vtable,
        post: *const bdr_group_trainer_post,
        observer: Option<
            unsafe extern "C" fn(ctx: *mut c_void, member: u32, env_steps: u64, opt_steps: u64, event: i32, scalars: *const f32, n_scalars: i32),
        >,
        observer_ctx: *mut c_void,
        out: *mut bdr_trainer_stats,
    ) -> i32;
    pub fn bdr_evaluator_default(ev: *mut bdr_evaluator, agent: *mut bdr_agent);
    pub fn bdr_evaluate(ev: *const bdr_evaluator, agent: *mut c_void, out: *mut bdr_eval_result) -> i32;
    pub fn bdr_trainer_post_default(post: *mut bdr_trainer_post);
    pub fn bdr_trainer_train_post(
        c: *const bdr_trainer_config,
        ops: *const bdr_trainer_ops,
        env: *const bdr_env_vtable,
        post: *const bdr_trainer_post,
        observer: bdr_trainer_observer,
        observer_ctx: *mut c_void,
        out: *mut bdr_trainer_stats,
    ) -> i32;
    pub fn bdr_trainer_train_offline_post(
        c: *const bdr_trainer_config,
        ops: *const bdr_trainer_ops,
        post: *const bdr_trainer_post,
        observer: bdr_trainer_observer,
        observer_ctx: *mut c_void,
        out: *mut bdr_trainer_stats,
    ) -> i32;
    pub fn bdr_agent_set_act_path(a: *mut bdr_agent, path: i32) -> i32;
    pub fn bdr_agent_hyper_get(a: *mut bdr_agent, id: i32, out: *mut f64) -> i32;
    pub fn bdr_agent_hyper_set(a: *mut bdr_agent, id: i32, v: f64) -> i32;
    pub fn bdr_bc_group_copy_members(g: *mut bdr_bc_group, src: *const u32, dst: *const u32, n: u32, flags: u32) -> i32;
    pub fn bdr_iql_group_copy_members(g: *mut bdr_iql_group, src: *const u32, dst: *const u32, n: u32, flags: u32) -> i32;
    pub fn bdr_awac_group_copy_members(g: *mut bdr_awac_group, src: *const u32, dst: *const u32, n: u32, flags: u32) -> i32;
    pub fn bdr_candle_sac_group_copy_members(g: *mut bdr_candle_sac_group, src: *const u32, dst: *const u32, n: u32, flags: u32) -> i32;
    pub fn bdr_candle_dqn_group_create(agents: *mut *const bdr_agent, n: u32, out: *mut *mut bdr_candle_dqn_group) -> i32;
    pub fn bdr_candle_dqn_group_destroy(g: *mut bdr_candle_dqn_group) -> i32;
    pub fn bdr_candle_dqn_group_size(g: *const bdr_candle_dqn_group, n: *mut u32) -> i32;
    pub fn bdr_candle_dqn_group_member(g: *const bdr_candle_dqn_group, i: u32, out: *mut *mut bdr_agent) -> i32;
    pub fn bdr_candle_dqn_group_info(g: *const bdr_candle_dqn_group, out: *mut bdr_group_info) -> i32;
    pub fn bdr_candle_dqn_group_opt(g: *mut bdr_candle_dqn_group, buffers: *mut *const bdr_replay) -> i32;
    pub fn bdr_candle_dqn_group_opt_with_scalars(g: *mut bdr_candle_dqn_group, buffers: *mut *const bdr_replay, out: *mut f32, cap_per_member: i32, n_out: *mut i32) -> i32;
    pub fn bdr_candle_dqn_group_sync(g: *mut bdr_candle_dqn_group) -> i32;
    pub fn bdr_candle_dqn_group_sample(
        g: *mut bdr_candle_dqn_group,
        norms: *mut *const bdr_obs_norm,
        n: u64,
        rows: *mut *const c_void,
        dtypes: *const i32,
        act_out: *mut *const i64,
    ) -> i32;
    pub fn bdr_candle_dqn_group_sample_members(
        g: *mut bdr_candle_dqn_group,
        members: *const u32,
        n_sel: u32,
        norms: *mut *const bdr_obs_norm,
        n: u64,
        rows: *mut *const c_void,
        dtypes: *const i32,
        act_out: *mut *const i64,
    ) -> i32;
    pub fn bdr_candle_dqn_group_last_q(g: *const bdr_candle_dqn_group, member: u32, q_out: *mut f32, n_floats: u64) -> i32;
    pub fn bdr_candle_dqn_group_push(
        g: *mut bdr_candle_dqn_group,
        buffers: *mut *const bdr_replay,
        n: u64,
        obs: *mut *const c_void,
        next_obs: *mut *const c_void,
        obs_dtypes: *const i32,
        act: *mut *const i64,
        reward: *mut *const f32,
        is_terminated: *mut *const i8,
        is_truncated: *mut *const i8,
    ) -> i32;
    pub fn bdr_candle_dqn_group_push_max_rows(g: *mut bdr_candle_dqn_group, buffers: *mut *const bdr_replay, obs_dtypes: *const i32, n_max: *mut u64) -> i32;
    pub fn bdr_candle_dqn_group_trainer_ops_default(ops: *mut bdr_group_trainer_ops, group: *mut bdr_candle_dqn_group, buffers: *mut *const bdr_replay);
    pub fn bdr_candle_dqn_group_eval_ops_default(ops: *mut bdr_group_eval_ops, group: *mut bdr_candle_dqn_group);
    pub fn bdr_candle_dqn_group_trainer_post_default(post: *mut bdr_group_trainer_post, group: *mut bdr_candle_dqn_group);
    pub fn bdr_agent_sample_raw(
        a: *mut bdr_agent,
        norm: *const bdr_obs_norm,
        n: u64,
        rows: *const c_void,
        dtype: i32,
        on_device: i32,
        row_stride: u64,
        act_out: *mut f32,
        idx_out: *mut i64,
    ) -> i32;
    pub fn bdr_trainer_train_offline(
        c: *const bdr_trainer_config,
        ops: *const bdr_trainer_ops,
        observer: bdr_trainer_observer,
        observer_ctx: *mut c_void,
        out: *mut bdr_trainer_stats,
    ) -> i32;

    // ---- async trainer
    pub fn bdr_model_mailbox_create(device: i32, n_floats: u64, n_readers: u32, out: *mut *mut bdr_model_mailbox) -> i32;
    pub fn bdr_model_mailbox_destroy(m: *mut bdr_model_mailbox) -> i32;
    pub fn bdr_agent_publish_model(a: *mut bdr_agent, which: i32, m: *mut bdr_model_mailbox, n_opts: u64) -> i32;
    pub fn bdr_agent_sync_model_from(
        a: *mut bdr_agent,
        which: i32,
        m: *mut bdr_model_mailbox,
        reader: u32,
        first: i32,
        n_opts_inout: *mut u64,
        updated: *mut i32,
    ) -> i32;
    pub fn bdr_async_trainer_config_default(c: *mut bdr_async_trainer_config);
    pub fn bdr_learner_ops_default(ops: *mut bdr_learner_ops, agent: *mut bdr_agent, buffer: *mut bdr_replay, mailbox: *mut bdr_model_mailbox);
    pub fn bdr_actor_ops_default(ops: *mut bdr_actor_ops, agent: *mut bdr_agent, mailbox: *mut bdr_model_mailbox, env: *const bdr_env_vtable);
    pub fn bdr_async_train(
        c: *const bdr_async_trainer_config,
        learner: *const bdr_learner_ops,
        actors: *const bdr_actor_ops,
        n_actors: u32,
        observer: bdr_async_observer,
        observer_ctx: *mut c_void,
        out: *mut bdr_async_stats,
        actor_stats: *mut bdr_actor_stat,
    ) -> i32;

    // ---- Atari frame preprocessing
    pub fn bdr_atari_prep_create(device: i32, n_envs: u32, width: u32, height: u32, out: *mut *mut bdr_atari_prep) -> i32;
    pub fn bdr_atari_prep_destroy(h: *mut bdr_atari_prep) -> i32;
    pub fn bdr_atari_prep_reset(h: *mut bdr_atari_prep, n: u32, env_ixs: *const u32, frames: *const u8) -> i32;
    pub fn bdr_atari_prep_step(h: *mut bdr_atari_prep, n: u32, env_ixs: *const u32, frames_a: *const u8, frames_b: *const u8) -> i32;
    pub fn bdr_atari_prep_obs(h: *mut bdr_atari_prep, n: u32, env_ixs: *const u32, obs_out: *mut u8) -> i32;
    pub fn bdr_atari_prep_device_stacks(h: *mut bdr_atari_prep, stacks: *mut *const u8) -> i32;
    pub fn bdr_atari_prep_copy_stack(h: *mut bdr_atari_prep, env_ix: u32, dst_dev: *mut c_void) -> i32;
    pub fn bdr_atari_prep_device_prev_stacks(h: *mut bdr_atari_prep, prev: *mut *const u8) -> i32;
    pub fn bdr_atari_clip_reward(r: f32, train: i32) -> f32;

    // ---- checkpoints, probes, profiling
    pub fn bdr_checkpoint_write(path: *const c_char, meta: *const bdr_named_tensor, n_tensors: u32, data: *const f32, n: u64) -> i32;
    pub fn bdr_checkpoint_read(path: *const c_char, meta: *const bdr_named_tensor, n_tensors: u32, data: *mut f32, n: u64) -> i32;
    pub fn bdr_dqn_probe(a: *mut bdr_agent, what: i32, out: *mut f32, n: u64) -> i32;
    pub fn bdr_dqn_mlp_layer_probe(a: *mut bdr_agent, buf: i32, z: i32, layer: i32, out: *mut f32, n: u64) -> i32;
    pub fn bdr_sac_probe(a: *mut bdr_agent, what: i32, out: *mut f32, n: u64) -> i32;
    pub fn bdr_agent_profile_enable(a: *mut bdr_agent, on: i32) -> i32;
    pub fn bdr_agent_profile_read(a: *mut bdr_agent, names_out: *mut c_char, names_cap: u64, ms_out: *mut f32, count_inout: *mut u64) -> i32;

    // ---- IQN
    pub fn bdr_iqn_config_default(cfg: *mut bdr_iqn_config);
    pub fn bdr_iqn_create(cfg: *const bdr_iqn_config, out: *mut *mut bdr_agent) -> i32;
    pub fn bdr_iqn_update_on_batch(
        a: *mut bdr_agent,
        n: u64,
        obs: *const c_void,
        act: *const i64,
        next_obs: *const c_void,
        reward: *const f32,
        is_terminated: *const i8,
        tau_pred: *const f32,
        n_pred: i32,
        tau_tgt: *const f32,
        n_tgt: i32,
        loss_out: *mut f32,
    ) -> i32;
    pub fn bdr_iqn_forward(a: *mut bdr_agent, which: i32, n: u64, obs: *const c_void, tau: *const f32, n_tau: i32, z_out: *mut f32) -> i32;
    pub fn bdr_iqn_qvalues(a: *mut bdr_agent, n: u64, obs: *const c_void, q_out: *mut f32, argmax_out: *mut i64) -> i32;
    pub fn bdr_iqn_probe(a: *mut bdr_agent, what: i32, out: *mut f32, n: u64) -> i32;

    // ---- SAC
    pub fn bdr_sac_config_default(cfg: *mut bdr_sac_config);
    pub fn bdr_sac_create(cfg: *const bdr_sac_config, out: *mut *mut bdr_agent) -> i32;
    pub fn bdr_sac_update_on_batch(
        a: *mut bdr_agent,
        n: u64,
        obs: *const f32,
        act: *const f32,
        next_obs: *const f32,
        reward: *const f32,
        is_terminated: *const i8,
        z_actor: *const f32,
        z_next: *const f32,
        rec3: *mut f32,
    ) -> i32;
    pub fn bdr_sac_keep_layers(a: *mut bdr_agent, on: i32) -> i32;
    pub fn bdr_sac_layer_probe(a: *mut bdr_agent, phase: i32, buf: i32, critic: i32, layer: i32, out: *mut f32, n: u64) -> i32;
    pub fn bdr_sac_sample(a: *mut bdr_agent, n: u64, obs: *const f32, act_out: *mut f32) -> i32;
    pub fn bdr_sac_sample_device(a: *mut bdr_agent, n: u64, obs_dev: *const c_void, row_stride: u64, act_out: *mut f32) -> i32;

    // ---- IQL (border-candle-agent/src/iql)
    pub fn bdr_iql_config_default(cfg: *mut bdr_iql_config);
    pub fn bdr_iql_create(cfg: *const bdr_iql_config, out: *mut *mut bdr_agent) -> i32;
    pub fn bdr_iql_update_on_batch(
        a: *mut bdr_agent,
        n: u64,
        obs: *const f32,
        act: *const f32,
        next_obs: *const f32,
        reward: *const f32,
        is_terminated: *const i8,
        is_truncated: *const i8,
        rec3: *mut f32,
    ) -> i32;
    pub fn bdr_iql_probe(a: *mut bdr_agent, what: i32, out: *mut f32, n: u64) -> i32;
    pub fn bdr_iql_sample(a: *mut bdr_agent, n: u64, obs: *const f32, act_out: *mut f32) -> i32;
    pub fn bdr_iql_sample_device(a: *mut bdr_agent, n: u64, obs_dev: *const c_void, row_stride: u64, act_out: *mut f32) -> i32;

    // ---- AWAC (border-candle-agent/src/awac)
    pub fn bdr_awac_config_default(cfg: *mut bdr_awac_config);
    pub fn bdr_awac_create(cfg: *const bdr_awac_config, out: *mut *mut bdr_agent) -> i32;
    pub fn bdr_awac_update_on_batch(
        a: *mut bdr_agent,
        n: u64,
        obs: *const f32,
        act: *const f32,
        next_obs: *const f32,
        reward: *const f32,
        is_terminated: *const i8,
        is_truncated: *const i8,
        z_pi: *const f32,
        z_next: *const f32,
        rec8: *mut f32,
    ) -> i32;
    pub fn bdr_awac_probe(a: *mut bdr_agent, what: i32, out: *mut f32, n: u64) -> i32;
    pub fn bdr_awac_sample(a: *mut bdr_agent, n: u64, obs: *const f32, act_out: *mut f32) -> i32;
    pub fn bdr_awac_sample_device(a: *mut bdr_agent, n: u64, obs_dev: *const c_void, row_stride: u64, act_out: *mut f32) -> i32;

    // ---- SAC of border-candle-agent (border-candle-agent/src/sac)
    pub fn bdr_candle_sac_config_default(cfg: *mut bdr_candle_sac_config);
    pub fn bdr_candle_sac_create(cfg: *const bdr_candle_sac_config, out: *mut *mut bdr_agent) -> i32;
    pub fn bdr_candle_sac_update_on_batch(
        a: *mut bdr_agent,
        n: u64,
        obs: *const f32,
        act: *const f32,
        next_obs: *const f32,
        reward: *const f32,
        is_terminated: *const i8,
        is_truncated: *const i8,
        z_pi: *const f32,
        z_next: *const f32,
        rec3: *mut f32,
    ) -> i32;
    pub fn bdr_candle_sac_probe(a: *mut bdr_agent, what: i32, out: *mut f32, n: u64) -> i32;
    pub fn bdr_candle_sac_sample(a: *mut bdr_agent, n: u64, obs: *const f32, act_out: *mut f32) -> i32;
    pub fn bdr_candle_sac_sample_device(a: *mut bdr_agent, n: u64, obs_dev: *const c_void, row_stride: u64, act_out: *mut f32) -> i32;

    // ---- DQN of border-candle-agent (border-candle-agent/src/dqn), Mlp Q-network
    pub fn bdr_candle_dqn_config_default(cfg: *mut bdr_candle_dqn_config);
    pub fn bdr_candle_dqn_create(cfg: *const bdr_candle_dqn_config, out: *mut *mut bdr_agent) -> i32;
    pub fn bdr_candle_dqn_update_on_batch(
        a: *mut bdr_agent,
        n: u64,
        obs: *const f32,
        act: *const i64,
        next_obs: *const f32,
        reward: *const f32,
        is_terminated: *const i8,
        is_truncated: *const i8,
        rec: *mut bdr_dqn_record,
    ) -> i32;
    pub fn bdr_candle_dqn_probe(a: *mut bdr_agent, what: i32, out: *mut f32, n: u64) -> i32;
    pub fn bdr_candle_dqn_cnn_config_default(cfg: *mut bdr_candle_dqn_cnn_config);
    pub fn bdr_candle_dqn_cnn_create(cfg: *const bdr_candle_dqn_cnn_config, out: *mut *mut bdr_agent) -> i32;
    pub fn bdr_candle_dqn_cnn_update_on_batch(
        a: *mut bdr_agent,
        n: u64,
        obs: *const u8,
        act: *const i64,
        next_obs: *const u8,
        reward: *const f32,
        is_terminated: *const i8,
        is_truncated: *const i8,
        rec: *mut bdr_dqn_record,
    ) -> i32;

    // ---- BC (border-candle-agent/src/bc)
    pub fn bdr_bc_config_default(cfg: *mut bdr_bc_config);
    pub fn bdr_bc_create(cfg: *const bdr_bc_config, out: *mut *mut bdr_agent) -> i32;
    pub fn bdr_bc_update_on_batch(a: *mut bdr_agent, n: u64, obs: *const f32, act: *const f32, rec_out: *mut f32) -> i32;
    pub fn bdr_bc_probe(a: *mut bdr_agent, what: i32, out: *mut f32, n: u64) -> i32;
    pub fn bdr_bc_sample(a: *mut bdr_agent, n: u64, obs: *const f32, act_out: *mut f32, idx_out: *mut i64) -> i32;
    pub fn bdr_bc_sample_device(
        a: *mut bdr_agent,
        n: u64,
        obs_dev: *const c_void,
        row_stride: u64,
        act_out: *mut f32,
        idx_out: *mut i64,
    ) -> i32;

    // ---- multi-GPU parameter exchange (RCCL over xGMI)
    pub fn bdr_comm_get_unique_id(id: *mut u8) -> i32;
    pub fn bdr_comm_init_rank(id: *const u8, nranks: i32, rank: i32, device: i32, out: *mut *mut bdr_comm) -> i32;
    pub fn bdr_comm_destroy(c: *mut bdr_comm) -> i32;
    pub fn bdr_comm_agree(c: *mut bdr_comm, local_ok: i32, all_ok: *mut i32) -> i32;
    pub fn bdr_agent_allreduce_params(a: *mut bdr_agent, c: *mut bdr_comm, which: i32) -> i32;
    pub fn bdr_agent_set_grad_comm(a: *mut bdr_agent, c: *mut bdr_comm) -> i32;
    pub fn bdr_agent_broadcast_params(a: *mut bdr_agent, c: *mut bdr_comm, which: i32, root: i32) -> i32;
}
