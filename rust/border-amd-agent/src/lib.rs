//! border's DQN / IQN / SAC agents and `SimpleReplayBuffer` on MI355X.
//!
//! Drop-in for `border-tch-agent` on the opt-step path: the same border-core traits ([`Agent`](border_core::Agent),
//! [`Policy`](border_core::Policy), [`Configurable`](border_core::Configurable),
//! [`ReplayBufferBase`](border_core::ReplayBufferBase), [`ExperienceBufferBase`](border_core::ExperienceBufferBase)) and
//! border-async-trainer's [`SyncModel`](border_async_trainer::SyncModel), implemented over `libborder_amd.so` - hand-written
//! HIP kernels for gfx950 behind the C ABI of `include/border_amd.h`.  No tch, no candle: nothing here links libtorch.
//!
//! * [`AmdReplayBuffer`] - `SimpleReplayBuffer` (`border-core/src/generic_replay_buffer/base.rs`) as a ring in HBM; indices of
//!   `batch()` are those of `StdRng::seed_from_u64(seed)`, bit for bit.
//! * [`AmdDqn`], [`AmdIqn`], [`AmdSac`] - `border-tch-agent/src/{dqn,iqn,sac}/base.rs`; configs keep the reference's field names
//!   and serde layout ([`config`]), so the example YAML files load unchanged.
//! * [`AmdDqnGroup`] - a set of small `Mlp` [`AmdDqn`] agents whose `Agent::opt` runs as one kernel launch, one workgroup per member
//!   (`bdr_agent_group_*`); the members stay ordinary agents.  [`GroupEvaluator`]: one member's evaluator for the lockstep
//!   `AmdDqnGroup::evaluate` / `train_post` (`bdr_evaluate_group`, `bdr_trainer_train_group_post`).
//! * [`AmdIql`] - `border-candle-agent/src/iql/base.rs` (offline RL; [`IqlConfig`] deserialises the candle YAML names).
//! * [`AmdAwac`] - `border-candle-agent/src/awac/base.rs` (offline and online RL; [`AwacConfig`] likewise).
//! * [`AmdCandleSac`] - `border-candle-agent/src/sac/base.rs` (the candle SAC with its `Mlp2` Gaussian actor; [`CandleSacConfig`]
//!   likewise).
//! * [`AmdCandleDqn`] - `border-candle-agent/src/dqn/base.rs` (the candle DQN with an `Mlp` Q-network and the reference's
//!   `SmallRng` exploration stream; [`CandleDqnConfig`] likewise).
//! * [`AmdBc`] - `border-candle-agent/src/bc/base.rs` (behaviour cloning; [`BcConfig`] likewise).
//! * [`AmdObsNorm`], [`AmdReplayBuffer::push_episode`] - `border-minari`'s `PenConverter` statistics / normalisation and
//!   `MinariDataset::create_replay_buffer`'s episode push, on the device.
//! * [`AmdEvaluator`], [`TrainerPost`], [`SampleRaw`] - `DefaultEvaluator` / `MinariEvaluator` and `Trainer::post_process` behind
//!   `bdr_evaluate` and the `*_post` Trainer loops; `sample_raw` / `set_act_path` on the dense-agent agents (one-launch acting).
//! * [`train_async`] - `border-async-trainer/src/util.rs:31-92` on one GPU (learner + actors + device mailbox), with the
//!   optional cross-GPU exchange over RCCL ([`Comm`]).
//!
//! An example binary changes two type aliases (`examples/atari/dqn_atari_tch/src/main.rs:28-45`):
//! `type Agent_ = AmdDqn<Env, ObsBatch, ActBatch>; type ReplayBuffer_ = AmdReplayBuffer<ObsBatch, ActBatch>;`
//! and keeps its `Trainer::build(config).train(env, step_proc, &mut agent, &mut buffer, ...)` call.
pub mod async_trainer;
pub mod awac;
pub mod bc;
pub mod bytes;
pub mod candle_dqn;
pub mod candle_sac;
pub mod comm;
pub mod config;
pub mod dataset;
pub mod dqn;
pub mod error;
pub mod evaluator;
pub mod ffi;
pub mod group;
mod handle;
pub mod iql;
pub mod iqn;
pub mod replay;
pub mod sac;

pub use async_trainer::{train_async, AmdAsyncTrainStat};
pub use bytes::{ActFromRows, DiscreteAct, FloatAct, ObsRows, RowBatch};
pub use comm::Comm;
pub use config::{
    ActionLimit, Activation, CandleMlpConfig, CandleOptimizerConfig, GaussianActorConfig, MultiCriticConfig, ValueConfig,
    ActorConfig, AtariCnnConfig, CriticConfig, CriticLoss, Device, DqnConfig, DqnExplorer, DqnModelConfig, EntCoefMode, EpsilonGreedy,
    ActorKind, Arithmetic, AwacConfig, CandleDqnAtariCnnConfig, CandleDqnConfig, CandleDqnModelConfig, CandleSacConfig, BcActionType, BcConfig, BcKernelForm, BcModelConfig, IqlConfig, IqnConfig, IqnExplorer, IqnModelConfig, IqnSample, MlpConfig, OptimizerConfig, QNetConfig, SacConfig, Softmax,
};
pub use awac::AmdAwac;
pub use bc::AmdBc;
pub use candle_dqn::AmdCandleDqn;
pub use candle_sac::AmdCandleSac;
pub use dataset::{AmdObsNorm, ObsElem};
pub use dqn::AmdDqn;
pub use group::{AmdAwacGroup, AmdBcGroup, AmdCandleDqnGroup, AmdCandleSacGroup, AmdDqnGroup, AmdIqlGroup, GroupEvaluator};
pub use evaluator::{ActPath, AmdEvaluator, EvalResult, Hyper, SampleRaw, TrainerPost};
pub use iql::AmdIql;
pub use iqn::AmdIqn;
pub use replay::AmdReplayBuffer;
pub use sac::AmdSac;
