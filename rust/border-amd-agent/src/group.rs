//! A group of small `Mlp` DQN agents whose `Agent::opt` runs as ONE kernel launch, one workgroup per member
//! (`bdr_agent_group_*` of `include/border_amd.h`); acting, pushing one transition per member and the compiled online loop
//! (`bdr_trainer_train_group`) are one launch / one loop for all members too.
//!
//! A launch grouping, not an agent kind: the members are ordinary [`AmdDqn`] agents - every trait method keeps working on a
//! member ([`AmdDqnGroup::member_mut`]) and means what it meant - that enqueue on the group's stream, so member calls and group
//! calls stay ordered and may be mixed freely.  Results are bit for bit those of stepping the same agents one after the other.
use crate::{
    awac::AmdAwac,
    bc::AmdBc,
    bytes::{DiscreteAct, ObsRows, RowBatch},
    candle_dqn::AmdCandleDqn,
    candle_sac::AmdCandleSac,
    config::DqnConfig,
    dqn::AmdDqn,
    error::{check, expect},
    evaluator::EvalResult,
    ffi,
    iql::AmdIql,
    replay::AmdReplayBuffer,
};
use anyhow::{anyhow, Result};
use border_core::{
    record::{Record, RecordValue},
    Configurable, Env,
};
use std::ffi::CString;
use std::os::raw::{c_char, c_void};
use std::path::Path;

/// Owns its members: dropping the group destroys them (`bdr_agent_group_destroy`).
pub struct AmdDqnGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    g: *mut ffi::bdr_agent_group,
    members: Vec<AmdDqn<E, O, A>>,
}

// SAFETY: as `AgentHandle` - one HIP stream for the group and its members, all device work behind `&mut`.
unsafe impl<E: Env, O: RowBatch, A: RowBatch> Send for AmdDqnGroup<E, O, A> {}

impl<E, O, A> AmdDqnGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    /// Builds one agent per config and groups them.  Fails (naming the member and the reason) unless every config is an `Mlp`
    /// Q-network that takes the one-workgroup step for its batch size, on one device, without amsgrad, and all configs share
    /// `n_updates_per_opt`; the agents built so far are dropped then.
    pub fn build(configs: Vec<DqnConfig>) -> Result<Self> {
        let members: Vec<AmdDqn<E, O, A>> = configs.into_iter().map(AmdDqn::build).collect();
        Self::adopt(members)
    }

    /// Groups agents that already exist.  On failure the agents are dropped as ordinary agents.
    pub fn adopt(members: Vec<AmdDqn<E, O, A>>) -> Result<Self> {
        if members.is_empty() {
            return Err(anyhow!("a group needs at least one member"));
        }
        let mut hs: Vec<*const ffi::bdr_agent> = members.iter().map(|m| m.a.h as *const ffi::bdr_agent).collect();
        let mut g = std::ptr::null_mut();
        check(unsafe { ffi::bdr_agent_group_create(hs.as_mut_ptr(), hs.len() as u32, &mut g) })?;
        Ok(Self { g, members })
    }

    pub fn handle(&self) -> *mut ffi::bdr_agent_group {
        self.g
    }

    pub fn len(&self) -> usize {
        self.members.len()
    }

    pub fn is_empty(&self) -> bool {
        self.members.is_empty()
    }

    pub fn member(&self, i: usize) -> &AmdDqn<E, O, A> {
        &self.members[i]
    }

    /// A member as the ordinary agent it is (`Agent`, `Policy`, `SyncModel`, `save_params` ...).
    pub fn member_mut(&mut self, i: usize) -> &mut AmdDqn<E, O, A> {
        &mut self.members[i]
    }

    /// The group's form and launch counts (`bdr_agent_group_info`): `form` is `ffi::BDR_GROUP_FORM_ONE_WORKGROUP` (every member takes
    /// the one-workgroup step: one launch per update round) or `ffi::BDR_GROUP_FORM_LAYERS` (members of one shape beyond it, such
    /// as Mlp[256, 256] at batch 64: the layer path's launch sequence of one member, each launch serving all members);
    /// `launches_per_round` the kernel launches of one update round on uniform rings, `kernel_launches` those the group's own
    /// calls have enqueued since it was created.
    pub fn info(&self) -> Result<ffi::bdr_group_info> {
        let mut out = ffi::bdr_group_info::default();
        check(unsafe { ffi::bdr_agent_group_info(self.g, &mut out) })?;
        Ok(out)
    }

    /// Prioritized replay under the group (`bdr_agent_group_set_prioritized`): switched on, `opt`, `opt_with_record`, `push` and
    /// `train` accept buffers built with a `PerConfig` - sampling, importance weights and `update_priority` of all prioritized
    /// members run as a fixed number of launches per round, bit for bit what the members' own calls give.  Off (the default), a
    /// prioritized buffer is refused.
    pub fn set_prioritized(&mut self, on: bool) -> Result<()> {
        check(unsafe { ffi::bdr_agent_group_set_prioritized(self.g, on as i32) })
    }

    fn buffer_handles(&self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<Vec<*const ffi::bdr_replay>> {
        if buffers.len() != self.members.len() {
            return Err(anyhow!("{} members need {} buffers, got {}", self.members.len(), self.members.len(), buffers.len()));
        }
        Ok(buffers.iter().map(|b| b.h as *const ffi::bdr_replay).collect())
    }

    /// `Agent::opt` of every member, member `i` on `buffers[i]`: `n_updates_per_opt` launches in all; only enqueues.
    /// A refused call (a prioritized, empty or mismatched buffer) leaves every member and every buffer where it was.
    pub fn opt(&mut self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<()> {
        let mut hs = self.buffer_handles(buffers)?;
        check(unsafe { ffi::bdr_agent_group_opt(self.g, hs.as_mut_ptr()) })
    }

    /// `Agent::opt_with_record` of every member: the same step, one synchronisation, the members' `Record`s in member order.
    pub fn opt_with_record(&mut self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<Vec<Record>> {
        const CAP: usize = 256;
        let mut hs = self.buffer_handles(buffers)?;
        let n = self.members.len();
        let mut vals = vec![0f32; n * CAP];
        let mut counts = vec![0i32; n];
        check(unsafe { ffi::bdr_agent_group_opt_with_scalars(self.g, hs.as_mut_ptr(), vals.as_mut_ptr(), CAP as i32, counts.as_mut_ptr()) })?;
        let mut out = Vec::with_capacity(n);
        for (i, m) in self.members.iter_mut().enumerate() {
            let keys = m.a.record_keys().to_vec();
            let mut record = Record::empty();
            for (k, v) in keys.iter().zip(vals[i * CAP..].iter().take(counts[i] as usize)) {
                record.insert(k.clone(), RecordValue::Scalar(*v));
            }
            out.push(record);
        }
        Ok(out)
    }

    fn row_pointers(&self, rows: &[&[f32]]) -> Result<Vec<*const c_void>> {
        if rows.len() != self.members.len() {
            return Err(anyhow!("{} members need {} observation rows, got {}", self.members.len(), self.members.len(), rows.len()));
        }
        Ok(rows.iter().map(|r| r.as_ptr() as *const c_void).collect())
    }

    /// `Policy::sample` of every member on one observation row each (`rows[i]`: the `in_dim` floats of member `i`), one launch;
    /// each member's exploration stream and counters advance exactly as its own `sample` advances them.
    pub fn sample(&mut self, rows: &[&[f32]]) -> Result<Vec<i64>> {
        let mut ptrs = self.row_pointers(rows)?;
        let mut act = vec![0i64; rows.len()];
        check(unsafe { ffi::bdr_agent_group_sample(self.g, ptrs.as_mut_ptr(), act.as_mut_ptr(), std::ptr::null_mut()) })?;
        Ok(act)
    }

    /// `Policy::sample` of the members `members` (strictly ascending indices) only, one launch of `members.len()` workgroups
    /// (`bdr_agent_group_sample_members`).  `rows` is still one row per member and the result has one entry per member, of which
    /// only the selected ones are written (the others are 0).  A member that is not selected is not touched: its exploration
    /// stream and counters stay where they were.
    pub fn sample_members(&mut self, members: &[u32], rows: &[&[f32]]) -> Result<Vec<i64>> {
        let mut ptrs = self.row_pointers(rows)?;
        let mut act = vec![0i64; rows.len()];
        check(unsafe {
            ffi::bdr_agent_group_sample_members(self.g, members.as_ptr(), members.len() as u32, ptrs.as_mut_ptr(), act.as_mut_ptr(), std::ptr::null_mut())
        })?;
        Ok(act)
    }

    /// `qnet.forward` of one observation row per member, one launch: member `i`'s action values.
    pub fn qvalues(&mut self, rows: &[&[f32]], n_actions: &[usize]) -> Result<Vec<Vec<f32>>> {
        let mut ptrs = self.row_pointers(rows)?;
        if n_actions.len() != rows.len() {
            return Err(anyhow!("n_actions: one entry per member"));
        }
        let mut q: Vec<Vec<f32>> = n_actions.iter().map(|&a| vec![0f32; a]).collect();
        let mut outs: Vec<*const f32> = q.iter_mut().map(|v| v.as_mut_ptr() as *const f32).collect();
        check(unsafe { ffi::bdr_agent_group_qvalues(self.g, ptrs.as_mut_ptr(), outs.as_mut_ptr()) })?;
        Ok(q)
    }

    /// `ExperienceBufferBase::push` of ONE transition per member, member `i`'s into `buffers[i]` at its head: one launch, no copy
    /// command.  `obs[i]` / `next_obs[i]`: the `in_dim` floats of member `i`; `act`, `reward` and the flags: one value per member.
    /// Each ring ends up exactly as its own `push` of that one transition leaves it.  A refused call (a prioritized ring, a
    /// single-frame store, a row width other than the member's, two members on one ring) moves nothing.
    pub fn push(
        &mut self,
        buffers: &mut [AmdReplayBuffer<O, A>],
        obs: &[&[f32]],
        act: &[i64],
        next_obs: &[&[f32]],
        reward: &[f32],
        is_terminated: &[i8],
        is_truncated: &[i8],
    ) -> Result<()> {
        let mut hs = self.buffer_handles(buffers)?;
        let mut o = self.row_pointers(obs)?;
        let mut x = self.row_pointers(next_obs)?;
        let n = self.members.len();
        if act.len() != n || reward.len() != n || is_terminated.len() != n || is_truncated.len() != n {
            return Err(anyhow!("{} members need {} actions, rewards and flags", n, n));
        }
        check(unsafe {
            ffi::bdr_agent_group_push(
                self.g,
                hs.as_mut_ptr(),
                o.as_mut_ptr(),
                act.as_ptr(),
                x.as_mut_ptr(),
                reward.as_ptr(),
                is_terminated.as_ptr(),
                is_truncated.as_ptr(),
            )
        })
    }

    /// `Trainer::train` (`trainer.rs:267-327`) for all members in lockstep, member `i` on `envs[i]` and `buffers[i]`, in the
    /// compiled loop `bdr_trainer_train_group`: one group sample, one group push and at most one group opt per iteration.
    /// `config.obs_row_bytes` is ignored (member `i`'s row is `obs_row_bytes[i]`); `config.act_row_bytes` must be 8.
    /// Returns one statistics block per member.
    pub fn train(
        &mut self,
        envs: &mut [E],
        buffers: &mut [AmdReplayBuffer<O, A>],
        obs_row_bytes: &[u64],
        config: &ffi::bdr_trainer_config,
    ) -> Result<Vec<ffi::bdr_trainer_stats>>
    where
        E::Obs: ObsRows,
        E::Act: DiscreteAct,
    {
        let n = self.members.len();
        if envs.len() != n || obs_row_bytes.len() != n {
            return Err(anyhow!("{} members need {} environments and row sizes", n, n));
        }
        let mut hs = self.buffer_handles(buffers)?;
        let mut ctxs: Vec<GroupEnvCtx<E>> =
            envs.iter_mut().zip(obs_row_bytes).map(|(e, &b)| GroupEnvCtx { env: e as *mut E, obs_row_bytes: b as usize }).collect();
        let vts = Self::env_vtables(&mut ctxs);
        let mut ops: ffi::bdr_group_trainer_ops = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_group_trainer_ops_default(&mut ops, self.g, hs.as_mut_ptr()) };
        let mut stats = vec![ffi::bdr_trainer_stats::default(); n];
        check(unsafe {
            ffi::bdr_trainer_train_group(config, obs_row_bytes.as_ptr(), &ops, vts.as_ptr(), None, std::ptr::null_mut(), stats.as_mut_ptr())
        })?;
        Ok(stats)
    }

    fn env_vtables(ctxs: &mut [GroupEnvCtx<E>]) -> Vec<ffi::bdr_env_vtable>
    where
        E::Obs: ObsRows,
        E::Act: DiscreteAct,
    {
        ctxs.iter_mut()
            .map(|c| ffi::bdr_env_vtable {
                ctx: c as *mut GroupEnvCtx<E> as *mut c_void,
                reset: Some(group_env_reset::<E>),
                step_with_reset: Some(group_env_step::<E>),
                obs_on_device: 0,
                device: 0,
            })
            .collect()
    }

    /// The Evaluator of every member in lockstep (`bdr_evaluate_group`): member `i` on `evaluators[i]`, one acting launch per round
    /// over the members that still have an episode open.  Each result is what a lone `bdr_evaluate` of that member gives; the
    /// members stay in the mode they are in.
    pub fn evaluate(&mut self, evaluators: &mut [GroupEvaluator<E>]) -> Result<Vec<EvalResult>>
    where
        E::Obs: ObsRows,
        E::Act: DiscreteAct,
    {
        let n = self.members.len();
        if evaluators.len() != n {
            return Err(anyhow!("{} members need {} evaluators, got {}", n, n, evaluators.len()));
        }
        let evs: Vec<ffi::bdr_evaluator> = evaluators.iter().map(|e| e.c).collect();
        // SAFETY: bdr_group_eval_ops_default fills every field.
        let mut ops: ffi::bdr_group_eval_ops = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_group_eval_ops_default(&mut ops, self.g) };
        let mut out = vec![ffi::bdr_eval_result::default(); n];
        check(unsafe { ffi::bdr_evaluate_group(evs.as_ptr(), &ops, out.as_mut_ptr()) })?;
        Ok(out.iter().map(eval_result).collect())
    }

    /// [`AmdDqnGroup::train`] plus `Trainer::post_process` per member (`bdr_trainer_train_group_post`): every `eval_interval` opt
    /// steps a lockstep evaluation on `evaluators`, member `i`'s best model in `model_dirs[i]/best`, and every `save_interval` opt
    /// steps every member in `model_dirs[i]/<opt_steps>`.  An interval of 0 means never.
    #[allow(clippy::too_many_arguments)]
    pub fn train_post(
        &mut self,
        envs: &mut [E],
        buffers: &mut [AmdReplayBuffer<O, A>],
        obs_row_bytes: &[u64],
        config: &ffi::bdr_trainer_config,
        evaluators: &mut [GroupEvaluator<E>],
        eval_interval: usize,
        save_interval: usize,
        model_dirs: &[&Path],
    ) -> Result<Vec<ffi::bdr_trainer_stats>>
    where
        E::Obs: ObsRows,
        E::Act: DiscreteAct,
    {
        let n = self.members.len();
        if envs.len() != n || obs_row_bytes.len() != n || model_dirs.len() != n {
            return Err(anyhow!("{} members need {} environments, row sizes and model directories", n, n));
        }
        if eval_interval > 0 && evaluators.len() != n {
            return Err(anyhow!("{} members need {} evaluators, got {}", n, n, evaluators.len()));
        }
        let mut hs = self.buffer_handles(buffers)?;
        let mut ctxs: Vec<GroupEnvCtx<E>> =
            envs.iter_mut().zip(obs_row_bytes).map(|(e, &b)| GroupEnvCtx { env: e as *mut E, obs_row_bytes: b as usize }).collect();
        let vts = Self::env_vtables(&mut ctxs);
        let mut ops: ffi::bdr_group_trainer_ops = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_group_trainer_ops_default(&mut ops, self.g, hs.as_mut_ptr()) };
        let evs: Vec<ffi::bdr_evaluator> = evaluators.iter().map(|e| e.c).collect();
        let mut dirs = Vec::with_capacity(n);
        for d in model_dirs {
            dirs.push(CString::new(d.to_string_lossy().as_bytes())?);
        }
        let mut dir_ptrs: Vec<*const c_char> = dirs.iter().map(|d| d.as_ptr()).collect();
        // SAFETY: bdr_group_trainer_post_default fills every field.
        let mut post: ffi::bdr_group_trainer_post = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_group_trainer_post_default(&mut post, self.g) };
        post.eval_interval = eval_interval as u64;
        post.save_interval = save_interval as u64;
        post.evaluators = if evs.is_empty() { std::ptr::null() } else { evs.as_ptr() };
        post.model_dirs = dir_ptrs.as_mut_ptr();
        let mut stats = vec![ffi::bdr_trainer_stats::default(); n];
        check(unsafe {
            ffi::bdr_trainer_train_group_post(
                config,
                obs_row_bytes.as_ptr(),
                &ops,
                vts.as_ptr(),
                &post,
                None,
                std::ptr::null_mut(),
                stats.as_mut_ptr(),
            )
        })?;
        Ok(stats)
    }

    /// Blocks until the group's stream is idle; device-side errors of any member surface here.
    pub fn sync(&mut self) -> Result<()> {
        check(unsafe { ffi::bdr_agent_group_sync(self.g) })
    }
}

fn eval_result(o: &ffi::bdr_eval_result) -> EvalResult {
    EvalResult {
        score: o.score,
        normalized: if o.has_normalized != 0 { Some(o.normalized) } else { None },
        n_steps: o.n_steps as usize,
        n_episodes: o.n_episodes as usize,
    }
}

// ---- a member's evaluation Env behind bdr_eval_env_vtable: f32 observation rows, one i64 action -----------------------------------
struct GroupEvalCtx<E: Env> {
    env: E,
    obs_row_bytes: usize,
}

/// One member's evaluator for [`AmdDqnGroup::evaluate`] / [`AmdDqnGroup::train_post`]: `DefaultEvaluator<E>`
/// (`default_evaluator.rs:64-88`) on an environment of its own with f32 observation rows of `obs_dim` elements and discrete actions.
pub struct GroupEvaluator<E: Env> {
    ctx: Box<GroupEvalCtx<E>>,
    c: ffi::bdr_evaluator,
}

impl<E> GroupEvaluator<E>
where
    E: Env,
    E::Obs: ObsRows,
    E::Act: DiscreteAct,
{
    pub fn new(env: E, n_episodes: usize, obs_dim: usize) -> Self {
        let obs_row_bytes = obs_dim * 4;
        let mut ctx = Box::new(GroupEvalCtx { env, obs_row_bytes });
        // SAFETY: bdr_evaluator_default fills every field of the struct it is handed.
        let mut c: ffi::bdr_evaluator = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_evaluator_default(&mut c, std::ptr::null_mut()) };
        c.n_episodes = n_episodes as u64;
        c.obs_row_bytes = obs_row_bytes as u64;
        c.act_row_bytes = 8;
        c.env = ffi::bdr_eval_env_vtable {
            ctx: &mut *ctx as *mut GroupEvalCtx<E> as *mut c_void,
            reset_with_index: Some(group_eval_reset::<E>),
            step: Some(group_eval_step::<E>),
            obs_on_device: 0,
            device: 0,
        };
        Self { ctx, c }
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
}

unsafe extern "C" fn group_eval_reset<E>(ctx: *mut c_void, ix: u64, obs_out: *mut c_void) -> i32
where
    E: Env,
    E::Obs: ObsRows,
{
    let ctx = &mut *(ctx as *mut GroupEvalCtx<E>);
    let r = std::panic::catch_unwind(std::panic::AssertUnwindSafe(|| match ctx.env.reset_with_index(ix as usize) {
        Ok(obs) => write_row(&obs, obs_out, ctx.obs_row_bytes),
        Err(_) => 90,
    }));
    r.unwrap_or(90) // a panic must not unwind into C
}

unsafe extern "C" fn group_eval_step<E>(
    ctx: *mut c_void,
    act: *const c_void,
    obs_out: *mut c_void,
    reward: *mut f32,
    is_terminated: *mut i8,
    is_truncated: *mut i8,
) -> i32
where
    E: Env,
    E::Obs: ObsRows,
    E::Act: DiscreteAct,
{
    let ctx = &mut *(ctx as *mut GroupEvalCtx<E>);
    let r = std::panic::catch_unwind(std::panic::AssertUnwindSafe(|| {
        let a = <E::Act as crate::bytes::ActFromRows<i64>>::from_rows(vec![*(act as *const i64)], 1);
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

// ---- a member's Env behind bdr_env_vtable (the callbacks of async_trainer.rs on an environment that already exists) ------------
struct GroupEnvCtx<E: Env> {
    env: *mut E,
    obs_row_bytes: usize,
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

unsafe extern "C" fn group_env_reset<E>(ctx: *mut c_void, obs_out: *mut c_void) -> i32
where
    E: Env,
    E::Obs: ObsRows,
{
    let ctx = &mut *(ctx as *mut GroupEnvCtx<E>);
    let r = std::panic::catch_unwind(std::panic::AssertUnwindSafe(|| match (*ctx.env).reset(None) {
        Ok(obs) => write_row(&obs, obs_out, ctx.obs_row_bytes),
        Err(_) => 90,
    }));
    r.unwrap_or(90) // a panic must not unwind into C
}

unsafe extern "C" fn group_env_step<E>(
    ctx: *mut c_void,
    act: *const c_void,
    obs_out: *mut c_void,
    reward: *mut f32,
    is_terminated: *mut i8,
    is_truncated: *mut i8,
    init_obs_out: *mut c_void,
) -> i32
where
    E: Env,
    E::Obs: ObsRows,
    E::Act: DiscreteAct,
{
    let ctx = &mut *(ctx as *mut GroupEnvCtx<E>);
    let r = std::panic::catch_unwind(std::panic::AssertUnwindSafe(|| {
        let a = <E::Act as crate::bytes::ActFromRows<i64>>::from_rows(vec![*(act as *const i64)], 1);
        let (step, _record) = (*ctx.env).step_with_reset(&a);
        let rc = write_row(&step.obs, obs_out, ctx.obs_row_bytes);
        if rc != ffi::BDR_OK {
            return rc;
        }
        *reward = step.reward[0];
        *is_terminated = step.is_terminated[0];
        *is_truncated = step.is_truncated[0];
        if step.is_done() {
            match &step.init_obs {
                Some(o) => return write_row(o, init_obs_out, ctx.obs_row_bytes),
                None => return 91,
            }
        }
        ffi::BDR_OK
    }));
    r.unwrap_or(91)
}

impl<E, O, A> Drop for AmdDqnGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    fn drop(&mut self) {
        expect(unsafe { ffi::bdr_agent_group_destroy(self.g) }, "bdr_agent_group_destroy");
        for m in self.members.iter_mut() {
            m.a.h = std::ptr::null_mut(); // destroyed with the group; bdr_agent_destroy(NULL) in the member's own drop is a no-op
        }
    }
}

/// A group of BC agents of one shape whose `Agent::opt` runs as the launch sequence of ONE member, every launch serving all members
/// (`bdr_bc_group_*`): 2L + 4 launches per round for L layers in the general kernel form, 2L + 2 with the MFMA head, whatever the
/// number of members.  The members may differ in seed, learning rate and optimizer; member `i` steps on `buffers[i]`, a uniform
/// buffer of its own or a view of one ([`AmdReplayBuffer::view`]), so that P members hold one copy of a dataset.
///
/// A launch grouping, not an agent kind: the members are ordinary [`AmdBc`] agents ([`AmdBcGroup::member_mut`]) on the group's
/// stream.  Results are bit for bit those of stepping the same agents one after the other.  Owns its members: dropping the group
/// destroys them (`bdr_bc_group_destroy`).
pub struct AmdBcGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    g: *mut ffi::bdr_bc_group,
    members: Vec<AmdBc<E, O, A>>,
}

// SAFETY: as `AgentHandle` - one HIP stream for the group and its members, all device work behind `&mut`.
unsafe impl<E: Env, O: RowBatch, A: RowBatch> Send for AmdBcGroup<E, O, A> {}

impl<E, O, A> AmdBcGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    /// Groups agents that already exist.  Fails, naming the first member concerned and the reason, unless all members are Continuous
    /// BC agents of one shape and one resolved kernel form (not the LDS head) on one device; the agents are then dropped as
    /// ordinary agents.
    pub fn adopt(members: Vec<AmdBc<E, O, A>>) -> Result<Self> {
        if members.is_empty() {
            return Err(anyhow!("a group needs at least one member"));
        }
        let mut hs: Vec<*const ffi::bdr_agent> = members.iter().map(|m| m.a.h as *const ffi::bdr_agent).collect();
        let mut g = std::ptr::null_mut();
        check(unsafe { ffi::bdr_bc_group_create(hs.as_mut_ptr(), hs.len() as u32, &mut g) })?;
        Ok(Self { g, members })
    }

    pub fn handle(&self) -> *mut ffi::bdr_bc_group {
        self.g
    }

    pub fn len(&self) -> usize {
        self.members.len()
    }

    pub fn is_empty(&self) -> bool {
        self.members.is_empty()
    }

    pub fn member(&self, i: usize) -> &AmdBc<E, O, A> {
        &self.members[i]
    }

    /// A member as the ordinary agent it is (`Agent`, `Policy`, `SyncModel`, `save_params` ...).
    pub fn member_mut(&mut self, i: usize) -> &mut AmdBc<E, O, A> {
        &mut self.members[i]
    }

    /// `bdr_bc_group_info`: `form` is `ffi::BDR_GROUP_FORM_BC_LAYERS`, `launches_per_round` the kernel launches of one update
    /// round, `kernel_launches` those the group's own calls have enqueued since it was created.
    pub fn info(&self) -> Result<ffi::bdr_group_info> {
        let mut out = ffi::bdr_group_info::default();
        check(unsafe { ffi::bdr_bc_group_info(self.g, &mut out) })?;
        Ok(out)
    }

    fn buffer_handles(&self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<Vec<*const ffi::bdr_replay>> {
        if buffers.len() != self.members.len() {
            return Err(anyhow!("{} members need {} buffers, got {}", self.members.len(), self.members.len(), buffers.len()));
        }
        Ok(buffers.iter().map(|b| b.h as *const ffi::bdr_replay).collect())
    }

    /// `Agent::opt` of every member, member `i` on `buffers[i]`; only enqueues.  A refused call (a prioritized, empty, mismatched
    /// or shared buffer) leaves every member and every buffer where it was.
    pub fn opt(&mut self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<()> {
        let mut hs = self.buffer_handles(buffers)?;
        check(unsafe { ffi::bdr_bc_group_opt(self.g, hs.as_mut_ptr()) })
    }

    /// `Agent::opt_with_record` of every member: the same round, one synchronisation, the members' `Record`s (`loss`) in member order.
    pub fn opt_with_record(&mut self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<Vec<Record>> {
        const CAP: usize = 8;
        let mut hs = self.buffer_handles(buffers)?;
        let n = self.members.len();
        let mut vals = vec![0f32; n * CAP];
        let mut counts = vec![0i32; n];
        check(unsafe { ffi::bdr_bc_group_opt_with_scalars(self.g, hs.as_mut_ptr(), vals.as_mut_ptr(), CAP as i32, counts.as_mut_ptr()) })?;
        let mut out = Vec::with_capacity(n);
        for (i, m) in self.members.iter_mut().enumerate() {
            let keys = m.a.record_keys().to_vec();
            let mut record = Record::empty();
            for (k, v) in keys.iter().zip(vals[i * CAP..].iter().take(counts[i] as usize)) {
                record.insert(k.clone(), RecordValue::Scalar(*v));
            }
            out.push(record);
        }
        Ok(out)
    }

    /// `Policy::sample` of every member in ONE launch (`bdr_bc_group_sample`): member `i` acts on the `n` rows of `rows[i]`
    /// (`n * obs_dim` f32 values, the same `n` for every member; two members may name the same slice) and gets `n * act_dim`
    /// actions, the bits of its own `bdr_agent_sample_raw`.  `norms[i]`: the normaliser of member `i`'s rows, or null; an empty
    /// slice means none for anybody.
    pub fn sample(&mut self, n: usize, rows: &[&[f32]], norms: &[*const ffi::bdr_obs_norm]) -> Result<Vec<Vec<f32>>> {
        self.sample_with(None, n, rows, norms)
    }

    /// The same for the members `members` (strictly ascending indices) only (`bdr_bc_group_sample_members`).  `rows` and the result
    /// still have one entry per member; the entries of members that are not selected are not read and stay empty.
    pub fn sample_members(&mut self, members: &[u32], n: usize, rows: &[&[f32]], norms: &[*const ffi::bdr_obs_norm]) -> Result<Vec<Vec<f32>>> {
        self.sample_with(Some(members), n, rows, norms)
    }

    fn sample_with(&mut self, members: Option<&[u32]>, n: usize, rows: &[&[f32]], norms: &[*const ffi::bdr_obs_norm]) -> Result<Vec<Vec<f32>>> {
        let p = self.members.len();
        if rows.len() != p || !(norms.is_empty() || norms.len() == p) {
            return Err(anyhow!("{} members need {} row slices and {} normalisers (or none), got {} and {}", p, p, p, rows.len(), norms.len()));
        }
        let act_dim = self.members[0].act_dim();
        let selected = |i: usize| members.map_or(true, |m| m.contains(&(i as u32)));
        let mut out: Vec<Vec<f32>> = (0..p).map(|i| if selected(i) { vec![0f32; n * act_dim] } else { Vec::new() }).collect();
        for i in (0..p).filter(|&i| selected(i)) {
            if n == 0 || rows[i].is_empty() || rows[i].len() % n != 0 {
                return Err(anyhow!("member {}: {} values are not {} rows of one width", i, rows[i].len(), n));
            }
        }
        let mut row_ptrs: Vec<*const c_void> = rows.iter().map(|r| r.as_ptr() as *const c_void).collect();
        let mut out_ptrs: Vec<*const f32> = out.iter_mut().map(|v| if v.is_empty() { std::ptr::null() } else { v.as_mut_ptr() as *const f32 }).collect();
        let mut norm_ptrs: Vec<*const ffi::bdr_obs_norm> = norms.to_vec();
        let norms_arg = if norm_ptrs.is_empty() { std::ptr::null_mut() } else { norm_ptrs.as_mut_ptr() };
        let dtypes = vec![ffi::BDR_DTYPE_F32; p];
        check(match members {
            None => unsafe { ffi::bdr_bc_group_sample(self.g, norms_arg, n as u64, row_ptrs.as_mut_ptr(), dtypes.as_ptr(), out_ptrs.as_mut_ptr()) },
            Some(m) => unsafe {
                ffi::bdr_bc_group_sample_members(
                    self.g,
                    m.as_ptr(),
                    m.len() as u32,
                    norms_arg,
                    n as u64,
                    row_ptrs.as_mut_ptr(),
                    dtypes.as_ptr(),
                    out_ptrs.as_mut_ptr(),
                )
            },
        })?;
        Ok(out)
    }

    /// `DefaultEvaluator` of every member in lockstep (`bdr_evaluate_bc_group`): member `i` on `evaluators[i]` - the C view of an
    /// evaluator of this crate with `act_row_bytes = 4 * act_dim`; f32 or float64 rows and a normaliser per member are allowed -
    /// with ONE acting launch per round over the members that still have an episode open.
    pub fn evaluate(&mut self, evaluators: &[ffi::bdr_evaluator]) -> Result<Vec<EvalResult>> {
        let n = self.members.len();
        if evaluators.len() != n {
            return Err(anyhow!("{} members need {} evaluators, got {}", n, n, evaluators.len()));
        }
        // SAFETY: bdr_bc_group_eval_ops_default fills every field.
        let mut ops: ffi::bdr_bc_group_eval_ops = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_bc_group_eval_ops_default(&mut ops, self.g) };
        let mut out = vec![ffi::bdr_eval_result::default(); n];
        check(unsafe { ffi::bdr_evaluate_bc_group(evaluators.as_ptr(), &ops, out.as_mut_ptr()) })?;
        Ok(out.iter().map(eval_result).collect())
    }

    /// `Trainer::train_offline` with `Trainer::post_process` for the group in compiled code
    /// (`bdr_trainer_train_offline_group_post`): `config.max_opts` update rounds, member `i` on `buffers[i]`; every `eval_interval`
    /// opt steps a lockstep evaluation on `evaluators`, member `i`'s best model in `model_dirs[i]/best`, every `save_interval` opt
    /// steps every member in `model_dirs[i]/<opt_steps>`.  An interval of 0 means never; with both 0, `evaluators` and `model_dirs`
    /// may be empty.
    pub fn train_offline(
        &mut self,
        buffers: &mut [AmdReplayBuffer<O, A>],
        config: &ffi::bdr_trainer_config,
        evaluators: &[ffi::bdr_evaluator],
        eval_interval: usize,
        save_interval: usize,
        model_dirs: &[&Path],
    ) -> Result<Vec<ffi::bdr_trainer_stats>> {
        let n = self.members.len();
        if (eval_interval > 0 && evaluators.len() != n) || ((eval_interval > 0 || save_interval > 0) && model_dirs.len() != n) {
            return Err(anyhow!("{} members need {} evaluators and model directories", n, n));
        }
        let mut hs = self.buffer_handles(buffers)?;
        let mut ops: ffi::bdr_group_trainer_ops = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_bc_group_trainer_ops_default(&mut ops, self.g, hs.as_mut_ptr()) };
        let mut dirs = Vec::with_capacity(n);
        for d in model_dirs {
            dirs.push(CString::new(d.to_string_lossy().as_bytes())?);
        }
        let mut dir_ptrs: Vec<*const c_char> = dirs.iter().map(|d| d.as_ptr()).collect();
        // SAFETY: bdr_bc_group_trainer_post_default fills every field.
        let mut post: ffi::bdr_bc_group_trainer_post = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_bc_group_trainer_post_default(&mut post, self.g) };
        post.eval_interval = eval_interval as u64;
        post.save_interval = save_interval as u64;
        post.evaluators = if evaluators.is_empty() { std::ptr::null() } else { evaluators.as_ptr() };
        post.model_dirs = if dir_ptrs.is_empty() { std::ptr::null_mut() } else { dir_ptrs.as_mut_ptr() };
        let mut stats = vec![ffi::bdr_trainer_stats::default(); n];
        check(unsafe { ffi::bdr_trainer_train_offline_group_post(config, &ops, &post, None, std::ptr::null_mut(), stats.as_mut_ptr()) })?;
        self.sync()?;
        Ok(stats)
    }

    /// Member `dst` becomes a copy of member `src` for every `(src, dst)` of `pairs`, ONE launch whatever their number
    /// (`bdr_bc_group_copy_members`); does not synchronise.  Every arena of the model table moves (networks and targets, the last
    /// gradient, exp_avg, exp_avg_sq) with the optimizer step counters, and with `hyper` every settable hyperparameter; the
    /// destination keeps its seed, noise counter, mode, act path, buffer and index stream, n_opts and best-model bookkeeping.
    /// Refused, naming the pair, before anything moves: an index out of range, `src == dst`, a destination listed twice, a member
    /// that is a destination in one pair and a source in another.  An empty list does nothing.
    pub fn copy_members(&mut self, pairs: &[(u32, u32)], hyper: bool) -> Result<()> {
        if pairs.is_empty() {
            return Ok(());
        }
        let src: Vec<u32> = pairs.iter().map(|p| p.0).collect();
        let dst: Vec<u32> = pairs.iter().map(|p| p.1).collect();
        let flags = if hyper { ffi::BDR_COPY_HYPER } else { 0 };
        check(unsafe { ffi::bdr_bc_group_copy_members(self.g, src.as_ptr(), dst.as_ptr(), pairs.len() as u32, flags) })
    }

    /// Waits for everything the group and its members have enqueued (`bdr_bc_group_sync`).
    pub fn sync(&mut self) -> Result<()> {
        check(unsafe { ffi::bdr_bc_group_sync(self.g) })
    }
}

impl<E, O, A> Drop for AmdBcGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    fn drop(&mut self) {
        expect(unsafe { ffi::bdr_bc_group_destroy(self.g) }, "bdr_bc_group_destroy");
        for m in self.members.iter_mut() {
            m.a.h = std::ptr::null_mut(); // destroyed with the group; bdr_agent_destroy(NULL) in the member's own drop is a no-op
        }
    }
}

/// A group of IQL agents of one shape whose `Agent::opt` (`Iql::opt_`, iql/base.rs:157-188) runs as the launch sequence of ONE member,
/// every launch serving all members (`bdr_iql_group_*`): 3 (Lq + Lv) + 2 Lp + 8 launches per round for Lv, Lq, Lp layers of value,
/// critic and actor, whatever the number of members.  The members may differ in seed, expectile, temperature, discount, the
/// critics' tau, advantage form, critic loss, action limit, learning rates and optimizers; member `i` steps on `buffers[i]`, a
/// uniform buffer of its own or a view of one ([`AmdReplayBuffer::view`]), so that P members hold one copy of a dataset.
///
/// A launch grouping, not an agent kind: the members are ordinary [`AmdIql`] agents ([`AmdIqlGroup::member_mut`]) on the group's
/// stream.  Results are bit for bit those of stepping the same agents one after the other.  Owns its members: dropping the group
/// destroys them (`bdr_iql_group_destroy`).
pub struct AmdIqlGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    g: *mut ffi::bdr_iql_group,
    members: Vec<AmdIql<E, O, A>>,
}

// SAFETY: as `AgentHandle` - one HIP stream for the group and its members, all device work behind `&mut`.
unsafe impl<E: Env, O: RowBatch, A: RowBatch> Send for AmdIqlGroup<E, O, A> {}

impl<E, O, A> AmdIqlGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    /// Groups agents that already exist.  Fails, naming the first member concerned and the reason, unless all members are IQL
    /// agents of one shape (obs and act dims, the three networks, at most two critics, batch size) with `n_updates_per_opt == 1`
    /// on one device; the agents are then dropped as ordinary agents.
    pub fn adopt(members: Vec<AmdIql<E, O, A>>) -> Result<Self> {
        if members.is_empty() {
            return Err(anyhow!("a group needs at least one member"));
        }
        let mut hs: Vec<*const ffi::bdr_agent> = members.iter().map(|m| m.a.h as *const ffi::bdr_agent).collect();
        let mut g = std::ptr::null_mut();
        check(unsafe { ffi::bdr_iql_group_create(hs.as_mut_ptr(), hs.len() as u32, &mut g) })?;
        Ok(Self { g, members })
    }

    pub fn handle(&self) -> *mut ffi::bdr_iql_group {
        self.g
    }

    pub fn len(&self) -> usize {
        self.members.len()
    }

    pub fn is_empty(&self) -> bool {
        self.members.is_empty()
    }

    pub fn member(&self, i: usize) -> &AmdIql<E, O, A> {
        &self.members[i]
    }

    /// A member as the ordinary agent it is (`Agent`, `Policy`, `SyncModel`, `save_params` ...).
    pub fn member_mut(&mut self, i: usize) -> &mut AmdIql<E, O, A> {
        &mut self.members[i]
    }

    /// `bdr_iql_group_info`: `form` is `ffi::BDR_GROUP_FORM_IQL_LAYERS`, `launches_per_round` the kernel launches of one update
    /// round, `kernel_launches` those the group's own calls have enqueued since it was created.
    pub fn info(&self) -> Result<ffi::bdr_group_info> {
        let mut out = ffi::bdr_group_info::default();
        check(unsafe { ffi::bdr_iql_group_info(self.g, &mut out) })?;
        Ok(out)
    }

    fn buffer_handles(&self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<Vec<*const ffi::bdr_replay>> {
        if buffers.len() != self.members.len() {
            return Err(anyhow!("{} members need {} buffers, got {}", self.members.len(), self.members.len(), buffers.len()));
        }
        Ok(buffers.iter().map(|b| b.h as *const ffi::bdr_replay).collect())
    }

    /// `Agent::opt` of every member, member `i` on `buffers[i]`; only enqueues.  A refused call (a prioritized, empty, mismatched
    /// or shared buffer) leaves every member and every buffer where it was.
    pub fn opt(&mut self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<()> {
        let mut hs = self.buffer_handles(buffers)?;
        check(unsafe { ffi::bdr_iql_group_opt(self.g, hs.as_mut_ptr()) })
    }

    /// `Agent::opt_with_record` of every member: the same round, one synchronisation, the members' `Record`s (`loss_value`,
    /// `loss_critic`, `loss_actor`) in member order.
    pub fn opt_with_record(&mut self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<Vec<Record>> {
        const CAP: usize = 8;
        let mut hs = self.buffer_handles(buffers)?;
        let n = self.members.len();
        let mut vals = vec![0f32; n * CAP];
        let mut counts = vec![0i32; n];
        check(unsafe { ffi::bdr_iql_group_opt_with_scalars(self.g, hs.as_mut_ptr(), vals.as_mut_ptr(), CAP as i32, counts.as_mut_ptr()) })?;
        let mut out = Vec::with_capacity(n);
        for (i, m) in self.members.iter_mut().enumerate() {
            let keys = m.a.record_keys().to_vec();
            let mut record = Record::empty();
            for (k, v) in keys.iter().zip(vals[i * CAP..].iter().take(counts[i] as usize)) {
                record.insert(k.clone(), RecordValue::Scalar(*v));
            }
            out.push(record);
        }
        Ok(out)
    }

    /// `Policy::sample` of every member in ONE launch (`bdr_iql_group_sample`): member `i` acts on the `n` rows of `rows[i]`
    /// (`n * obs_dim` f32 values, the same `n` for every member; two members may name the same slice) and gets `n * act_dim`
    /// actions, the bits of its own `bdr_agent_sample_raw` in its current mode at its current noise counter: a member in train mode
    /// takes `n * act_dim` draws of its noise stream, a member in eval mode none.  `norms[i]`: the normaliser of member `i`'s rows,
    /// or null; an empty slice means none for anybody.
    pub fn sample(&mut self, n: usize, rows: &[&[f32]], norms: &[*const ffi::bdr_obs_norm]) -> Result<Vec<Vec<f32>>> {
        self.sample_with(None, n, rows, norms)
    }

    /// The same for the members `members` (strictly ascending indices) only (`bdr_iql_group_sample_members`).  `rows` and the result
    /// still have one entry per member; the entries of members that are not selected are not read and stay empty, and their noise
    /// counters stay where they were.
    pub fn sample_members(&mut self, members: &[u32], n: usize, rows: &[&[f32]], norms: &[*const ffi::bdr_obs_norm]) -> Result<Vec<Vec<f32>>> {
        self.sample_with(Some(members), n, rows, norms)
    }

    fn sample_with(&mut self, members: Option<&[u32]>, n: usize, rows: &[&[f32]], norms: &[*const ffi::bdr_obs_norm]) -> Result<Vec<Vec<f32>>> {
        let p = self.members.len();
        if rows.len() != p || !(norms.is_empty() || norms.len() == p) {
            return Err(anyhow!("{} members need {} row slices and {} normalisers (or none), got {} and {}", p, p, p, rows.len(), norms.len()));
        }
        let act_dim = self.members[0].act_dim();
        let selected = |i: usize| members.map_or(true, |m| m.contains(&(i as u32)));
        let mut out: Vec<Vec<f32>> = (0..p).map(|i| if selected(i) { vec![0f32; n * act_dim] } else { Vec::new() }).collect();
        for i in (0..p).filter(|&i| selected(i)) {
            if n == 0 || rows[i].is_empty() || rows[i].len() % n != 0 {
                return Err(anyhow!("member {}: {} values are not {} rows of one width", i, rows[i].len(), n));
            }
        }
        let mut row_ptrs: Vec<*const c_void> = rows.iter().map(|r| r.as_ptr() as *const c_void).collect();
        let mut out_ptrs: Vec<*const f32> = out.iter_mut().map(|v| if v.is_empty() { std::ptr::null() } else { v.as_mut_ptr() as *const f32 }).collect();
        let mut norm_ptrs: Vec<*const ffi::bdr_obs_norm> = norms.to_vec();
        let norms_arg = if norm_ptrs.is_empty() { std::ptr::null_mut() } else { norm_ptrs.as_mut_ptr() };
        let dtypes = vec![ffi::BDR_DTYPE_F32; p];
        check(match members {
            None => unsafe { ffi::bdr_iql_group_sample(self.g, norms_arg, n as u64, row_ptrs.as_mut_ptr(), dtypes.as_ptr(), out_ptrs.as_mut_ptr()) },
            Some(m) => unsafe {
                ffi::bdr_iql_group_sample_members(
                    self.g,
                    m.as_ptr(),
                    m.len() as u32,
                    norms_arg,
                    n as u64,
                    row_ptrs.as_mut_ptr(),
                    dtypes.as_ptr(),
                    out_ptrs.as_mut_ptr(),
                )
            },
        })?;
        Ok(out)
    }

    /// `DefaultEvaluator` of every member in lockstep (`bdr_evaluate_bc_group` behind IQL's table): member `i` on `evaluators[i]` -
    /// the C view of an evaluator of this crate with `act_row_bytes = 4 * act_dim`; f32 or float64 rows and a normaliser per member
    /// are allowed - with ONE acting launch per round over the members that still have an episode open.
    pub fn evaluate(&mut self, evaluators: &[ffi::bdr_evaluator]) -> Result<Vec<EvalResult>> {
        let n = self.members.len();
        if evaluators.len() != n {
            return Err(anyhow!("{} members need {} evaluators, got {}", n, n, evaluators.len()));
        }
        // SAFETY: bdr_iql_group_eval_ops_default fills every field.
        let mut ops: ffi::bdr_bc_group_eval_ops = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_iql_group_eval_ops_default(&mut ops, self.g) };
        let mut out = vec![ffi::bdr_eval_result::default(); n];
        check(unsafe { ffi::bdr_evaluate_bc_group(evaluators.as_ptr(), &ops, out.as_mut_ptr()) })?;
        Ok(out.iter().map(eval_result).collect())
    }

    /// `Trainer::train_offline` with `Trainer::post_process` for the group in compiled code
    /// (`bdr_trainer_train_offline_group_post`): `config.max_opts` update rounds, member `i` on `buffers[i]`; every `eval_interval`
    /// opt steps a lockstep evaluation on `evaluators`, member `i`'s best model in `model_dirs[i]/best`, every `save_interval` opt
    /// steps every member in `model_dirs[i]/<opt_steps>`.  An interval of 0 means never; with both 0, `evaluators` and `model_dirs`
    /// may be empty.
    pub fn train_offline(
        &mut self,
        buffers: &mut [AmdReplayBuffer<O, A>],
        config: &ffi::bdr_trainer_config,
        evaluators: &[ffi::bdr_evaluator],
        eval_interval: usize,
        save_interval: usize,
        model_dirs: &[&Path],
    ) -> Result<Vec<ffi::bdr_trainer_stats>> {
        let n = self.members.len();
        if (eval_interval > 0 && evaluators.len() != n) || ((eval_interval > 0 || save_interval > 0) && model_dirs.len() != n) {
            return Err(anyhow!("{} members need {} evaluators and model directories", n, n));
        }
        let mut hs = self.buffer_handles(buffers)?;
        let mut ops: ffi::bdr_group_trainer_ops = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_iql_group_trainer_ops_default(&mut ops, self.g, hs.as_mut_ptr()) };
        let mut dirs = Vec::with_capacity(n);
        for d in model_dirs {
            dirs.push(CString::new(d.to_string_lossy().as_bytes())?);
        }
        let mut dir_ptrs: Vec<*const c_char> = dirs.iter().map(|d| d.as_ptr()).collect();
        // SAFETY: bdr_iql_group_trainer_post_default fills every field.
        let mut post: ffi::bdr_bc_group_trainer_post = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_iql_group_trainer_post_default(&mut post, self.g) };
        post.eval_interval = eval_interval as u64;
        post.save_interval = save_interval as u64;
        post.evaluators = if evaluators.is_empty() { std::ptr::null() } else { evaluators.as_ptr() };
        post.model_dirs = if dir_ptrs.is_empty() { std::ptr::null_mut() } else { dir_ptrs.as_mut_ptr() };
        let mut stats = vec![ffi::bdr_trainer_stats::default(); n];
        check(unsafe { ffi::bdr_trainer_train_offline_group_post(config, &ops, &post, None, std::ptr::null_mut(), stats.as_mut_ptr()) })?;
        self.sync()?;
        Ok(stats)
    }

    /// Member `dst` becomes a copy of member `src` for every `(src, dst)` of `pairs`, ONE launch whatever their number
    /// (`bdr_iql_group_copy_members`); does not synchronise.  Every arena of the model table moves (networks and targets, the last
    /// gradient, exp_avg, exp_avg_sq) with the optimizer step counters, and with `hyper` every settable hyperparameter; the
    /// destination keeps its seed, noise counter, mode, act path, buffer and index stream, n_opts and best-model bookkeeping.
    /// Refused, naming the pair, before anything moves: an index out of range, `src == dst`, a destination listed twice, a member
    /// that is a destination in one pair and a source in another.  An empty list does nothing.
    pub fn copy_members(&mut self, pairs: &[(u32, u32)], hyper: bool) -> Result<()> {
        if pairs.is_empty() {
            return Ok(());
        }
        let src: Vec<u32> = pairs.iter().map(|p| p.0).collect();
        let dst: Vec<u32> = pairs.iter().map(|p| p.1).collect();
        let flags = if hyper { ffi::BDR_COPY_HYPER } else { 0 };
        check(unsafe { ffi::bdr_iql_group_copy_members(self.g, src.as_ptr(), dst.as_ptr(), pairs.len() as u32, flags) })
    }

    /// Waits for everything the group and its members have enqueued (`bdr_iql_group_sync`).
    pub fn sync(&mut self) -> Result<()> {
        check(unsafe { ffi::bdr_iql_group_sync(self.g) })
    }
}

impl<E, O, A> Drop for AmdIqlGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    fn drop(&mut self) {
        expect(unsafe { ffi::bdr_iql_group_destroy(self.g) }, "bdr_iql_group_destroy");
        for m in self.members.iter_mut() {
            m.a.h = std::ptr::null_mut(); // destroyed with the group; bdr_agent_destroy(NULL) in the member's own drop is a no-op
        }
    }
}

/// A group of AWAC agents of one shape whose `Agent::opt` (`Awac::opt_`, awac/base.rs:170-215) runs as the launch sequence of ONE
/// member, every launch serving all members (`bdr_awac_group_*`): 3 (Lp + Lq) + 8 launches per round for Lp, Lq layers of actor and
/// critic, whatever the number of members.  The members may differ in seed, temperature, weight clip, discount, the critics' tau,
/// advantage form, critic loss, action limit, learning rates, optimizers and train / eval mode; member `i` steps on `buffers[i]`, a
/// uniform buffer of its own or a view of one ([`AmdReplayBuffer::view`]), so that P members hold one copy of a dataset.  A round
/// draws its noise inside the round: a member in train mode takes `2 * batch_size * act_dim` draws at its own noise counter, the
/// stream its own `sample` and the group's `sample` continue.
///
/// A launch grouping, not an agent kind: the members are ordinary [`AmdAwac`] agents ([`AmdAwacGroup::member_mut`]) on the group's
/// stream.  Results are bit for bit those of stepping the same agents one after the other.  Owns its members: dropping the group
/// destroys them (`bdr_awac_group_destroy`).
pub struct AmdAwacGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    g: *mut ffi::bdr_awac_group,
    members: Vec<AmdAwac<E, O, A>>,
}

// SAFETY: as `AgentHandle` - one HIP stream for the group and its members, all device work behind `&mut`.
unsafe impl<E: Env, O: RowBatch, A: RowBatch> Send for AmdAwacGroup<E, O, A> {}

impl<E, O, A> AmdAwacGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    /// Groups agents that already exist.  Fails, naming the first member concerned and the reason, unless all members are AWAC
    /// agents of one shape (obs and act dims, both networks, at most two critics, batch size) with `n_updates_per_opt == 1`
    /// on one device; the agents are then dropped as ordinary agents.
    pub fn adopt(members: Vec<AmdAwac<E, O, A>>) -> Result<Self> {
        if members.is_empty() {
            return Err(anyhow!("a group needs at least one member"));
        }
        let mut hs: Vec<*const ffi::bdr_agent> = members.iter().map(|m| m.a.h as *const ffi::bdr_agent).collect();
        let mut g = std::ptr::null_mut();
        check(unsafe { ffi::bdr_awac_group_create(hs.as_mut_ptr(), hs.len() as u32, &mut g) })?;
        Ok(Self { g, members })
    }

    pub fn handle(&self) -> *mut ffi::bdr_awac_group {
        self.g
    }

    pub fn len(&self) -> usize {
        self.members.len()
    }

    pub fn is_empty(&self) -> bool {
        self.members.is_empty()
    }

    pub fn member(&self, i: usize) -> &AmdAwac<E, O, A> {
        &self.members[i]
    }

    /// A member as the ordinary agent it is (`Agent`, `Policy`, `SyncModel`, `save_params` ...).
    pub fn member_mut(&mut self, i: usize) -> &mut AmdAwac<E, O, A> {
        &mut self.members[i]
    }

    /// `bdr_awac_group_info`: `form` is `ffi::BDR_GROUP_FORM_AWAC_LAYERS`, `launches_per_round` the kernel launches of one update
    /// round, `kernel_launches` those the group's own calls have enqueued since it was created.
    pub fn info(&self) -> Result<ffi::bdr_group_info> {
        let mut out = ffi::bdr_group_info::default();
        check(unsafe { ffi::bdr_awac_group_info(self.g, &mut out) })?;
        Ok(out)
    }

    fn buffer_handles(&self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<Vec<*const ffi::bdr_replay>> {
        if buffers.len() != self.members.len() {
            return Err(anyhow!("{} members need {} buffers, got {}", self.members.len(), self.members.len(), buffers.len()));
        }
        Ok(buffers.iter().map(|b| b.h as *const ffi::bdr_replay).collect())
    }

    /// `Agent::opt` of every member, member `i` on `buffers[i]`; only enqueues.  A refused call (a prioritized, empty, mismatched
    /// or shared buffer) leaves every member and every buffer where it was.
    pub fn opt(&mut self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<()> {
        let mut hs = self.buffer_handles(buffers)?;
        check(unsafe { ffi::bdr_awac_group_opt(self.g, hs.as_mut_ptr()) })
    }

    /// `Agent::opt_with_record` of every member: the same round, one synchronisation, the members' `Record`s (the eight
    /// keys of an AWAC record) in member order.
    pub fn opt_with_record(&mut self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<Vec<Record>> {
        const CAP: usize = 8;
        let mut hs = self.buffer_handles(buffers)?;
        let n = self.members.len();
        let mut vals = vec![0f32; n * CAP];
        let mut counts = vec![0i32; n];
        check(unsafe { ffi::bdr_awac_group_opt_with_scalars(self.g, hs.as_mut_ptr(), vals.as_mut_ptr(), CAP as i32, counts.as_mut_ptr()) })?;
        let mut out = Vec::with_capacity(n);
        for (i, m) in self.members.iter_mut().enumerate() {
            let keys = m.a.record_keys().to_vec();
            let mut record = Record::empty();
            for (k, v) in keys.iter().zip(vals[i * CAP..].iter().take(counts[i] as usize)) {
                record.insert(k.clone(), RecordValue::Scalar(*v));
            }
            out.push(record);
        }
        Ok(out)
    }

    /// `Policy::sample` of every member in ONE launch (`bdr_awac_group_sample`): member `i` acts on the `n` rows of `rows[i]`
    /// (`n * obs_dim` f32 values, the same `n` for every member; two members may name the same slice) and gets `n * act_dim`
    /// actions, the bits of its own `bdr_agent_sample_raw` in its current mode at its current noise counter: a member in train mode
    /// takes `n * act_dim` draws of its noise stream, a member in eval mode none.  `norms[i]`: the normaliser of member `i`'s rows,
    /// or null; an empty slice means none for anybody.
    pub fn sample(&mut self, n: usize, rows: &[&[f32]], norms: &[*const ffi::bdr_obs_norm]) -> Result<Vec<Vec<f32>>> {
        self.sample_with(None, n, rows, norms)
    }

    /// The same for the members `members` (strictly ascending indices) only (`bdr_awac_group_sample_members`).  `rows` and the result
    /// still have one entry per member; the entries of members that are not selected are not read and stay empty, and their noise
    /// counters stay where they were.
    pub fn sample_members(&mut self, members: &[u32], n: usize, rows: &[&[f32]], norms: &[*const ffi::bdr_obs_norm]) -> Result<Vec<Vec<f32>>> {
        self.sample_with(Some(members), n, rows, norms)
    }

    fn sample_with(&mut self, members: Option<&[u32]>, n: usize, rows: &[&[f32]], norms: &[*const ffi::bdr_obs_norm]) -> Result<Vec<Vec<f32>>> {
        let p = self.members.len();
        if rows.len() != p || !(norms.is_empty() || norms.len() == p) {
            return Err(anyhow!("{} members need {} row slices and {} normalisers (or none), got {} and {}", p, p, p, rows.len(), norms.len()));
        }
        let act_dim = self.members[0].act_dim();
        let selected = |i: usize| members.map_or(true, |m| m.contains(&(i as u32)));
        let mut out: Vec<Vec<f32>> = (0..p).map(|i| if selected(i) { vec![0f32; n * act_dim] } else { Vec::new() }).collect();
        for i in (0..p).filter(|&i| selected(i)) {
            if n == 0 || rows[i].is_empty() || rows[i].len() % n != 0 {
                return Err(anyhow!("member {}: {} values are not {} rows of one width", i, rows[i].len(), n));
            }
        }
        let mut row_ptrs: Vec<*const c_void> = rows.iter().map(|r| r.as_ptr() as *const c_void).collect();
        let mut out_ptrs: Vec<*const f32> = out.iter_mut().map(|v| if v.is_empty() { std::ptr::null() } else { v.as_mut_ptr() as *const f32 }).collect();
        let mut norm_ptrs: Vec<*const ffi::bdr_obs_norm> = norms.to_vec();
        let norms_arg = if norm_ptrs.is_empty() { std::ptr::null_mut() } else { norm_ptrs.as_mut_ptr() };
        let dtypes = vec![ffi::BDR_DTYPE_F32; p];
        check(match members {
            None => unsafe { ffi::bdr_awac_group_sample(self.g, norms_arg, n as u64, row_ptrs.as_mut_ptr(), dtypes.as_ptr(), out_ptrs.as_mut_ptr()) },
            Some(m) => unsafe {
                ffi::bdr_awac_group_sample_members(
                    self.g,
                    m.as_ptr(),
                    m.len() as u32,
                    norms_arg,
                    n as u64,
                    row_ptrs.as_mut_ptr(),
                    dtypes.as_ptr(),
                    out_ptrs.as_mut_ptr(),
                )
            },
        })?;
        Ok(out)
    }

    /// `DefaultEvaluator` of every member in lockstep (`bdr_evaluate_bc_group` behind AWAC's table): member `i` on `evaluators[i]` -
    /// the C view of an evaluator of this crate with `act_row_bytes = 4 * act_dim`; f32 or float64 rows and a normaliser per member
    /// are allowed - with ONE acting launch per round over the members that still have an episode open.
    pub fn evaluate(&mut self, evaluators: &[ffi::bdr_evaluator]) -> Result<Vec<EvalResult>> {
        let n = self.members.len();
        if evaluators.len() != n {
            return Err(anyhow!("{} members need {} evaluators, got {}", n, n, evaluators.len()));
        }
        // SAFETY: bdr_awac_group_eval_ops_default fills every field.
        let mut ops: ffi::bdr_bc_group_eval_ops = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_awac_group_eval_ops_default(&mut ops, self.g) };
        let mut out = vec![ffi::bdr_eval_result::default(); n];
        check(unsafe { ffi::bdr_evaluate_bc_group(evaluators.as_ptr(), &ops, out.as_mut_ptr()) })?;
        Ok(out.iter().map(eval_result).collect())
    }

    /// `Trainer::train_offline` with `Trainer::post_process` for the group in compiled code
    /// (`bdr_trainer_train_offline_group_post`): `config.max_opts` update rounds, member `i` on `buffers[i]`; every `eval_interval`
    /// opt steps a lockstep evaluation on `evaluators`, member `i`'s best model in `model_dirs[i]/best`, every `save_interval` opt
    /// steps every member in `model_dirs[i]/<opt_steps>`.  An interval of 0 means never; with both 0, `evaluators` and `model_dirs`
    /// may be empty.
    pub fn train_offline(
        &mut self,
        buffers: &mut [AmdReplayBuffer<O, A>],
        config: &ffi::bdr_trainer_config,
        evaluators: &[ffi::bdr_evaluator],
        eval_interval: usize,
        save_interval: usize,
        model_dirs: &[&Path],
    ) -> Result<Vec<ffi::bdr_trainer_stats>> {
        let n = self.members.len();
        if (eval_interval > 0 && evaluators.len() != n) || ((eval_interval > 0 || save_interval > 0) && model_dirs.len() != n) {
            return Err(anyhow!("{} members need {} evaluators and model directories", n, n));
        }
        let mut hs = self.buffer_handles(buffers)?;
        let mut ops: ffi::bdr_group_trainer_ops = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_awac_group_trainer_ops_default(&mut ops, self.g, hs.as_mut_ptr()) };
        let mut dirs = Vec::with_capacity(n);
        for d in model_dirs {
            dirs.push(CString::new(d.to_string_lossy().as_bytes())?);
        }
        let mut dir_ptrs: Vec<*const c_char> = dirs.iter().map(|d| d.as_ptr()).collect();
        // SAFETY: bdr_awac_group_trainer_post_default fills every field.
        let mut post: ffi::bdr_bc_group_trainer_post = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_awac_group_trainer_post_default(&mut post, self.g) };
        post.eval_interval = eval_interval as u64;
        post.save_interval = save_interval as u64;
        post.evaluators = if evaluators.is_empty() { std::ptr::null() } else { evaluators.as_ptr() };
        post.model_dirs = if dir_ptrs.is_empty() { std::ptr::null_mut() } else { dir_ptrs.as_mut_ptr() };
        let mut stats = vec![ffi::bdr_trainer_stats::default(); n];
        check(unsafe { ffi::bdr_trainer_train_offline_group_post(config, &ops, &post, None, std::ptr::null_mut(), stats.as_mut_ptr()) })?;
        self.sync()?;
        Ok(stats)
    }

    /// `ExperienceBufferBase::push` of `n` transitions per member, member `i`'s into `buffers[i]`, in ONE launch
    /// (`bdr_awac_group_push`); only enqueues.  `obs[i]` / `next_obs[i]`: `n * obs_dim` f32 values, `act[i]`: `n * act_dim`,
    /// `reward[i]`, `is_terminated[i]`, `is_truncated[i]`: `n` values.  Each ring ends up exactly as its own `push` of those rows
    /// leaves it (a push may cross the wrap).  `n` is bounded by one staging slot ([`Self::push_max_rows`]); a refused call (a
    /// view, a prioritized ring, a single-frame store, a row width other than the members', two members on one ring, too many
    /// rows) moves nothing.  float64 rows go through `ffi::bdr_awac_group_push` with `BDR_DTYPE_F64`.
    #[allow(clippy::too_many_arguments)]
    pub fn push(
        &mut self,
        buffers: &mut [AmdReplayBuffer<O, A>],
        n: usize,
        obs: &[&[f32]],
        act: &[&[f32]],
        next_obs: &[&[f32]],
        reward: &[&[f32]],
        is_terminated: &[&[i8]],
        is_truncated: &[&[i8]],
    ) -> Result<()> {
        let mut hs = self.buffer_handles(buffers)?;
        let p = self.members.len();
        if obs.len() != p || act.len() != p || next_obs.len() != p || reward.len() != p || is_terminated.len() != p || is_truncated.len() != p {
            return Err(anyhow!("{} members need {} slices of every field", p, p));
        }
        let (od, ad) = (self.members[0].obs_dim(), self.members[0].act_dim());
        for i in 0..p {
            if obs[i].len() != n * od || next_obs[i].len() != n * od || act[i].len() != n * ad {
                return Err(anyhow!("member {}: {} rows need {} observation and {} action values", i, n, n * od, n * ad));
            }
            if reward[i].len() != n || is_terminated[i].len() != n || is_truncated[i].len() != n {
                return Err(anyhow!("member {}: {} rows need {} rewards and flags", i, n, n));
            }
        }
        let mut o: Vec<*const c_void> = obs.iter().map(|r| r.as_ptr() as *const c_void).collect();
        let mut x: Vec<*const c_void> = next_obs.iter().map(|r| r.as_ptr() as *const c_void).collect();
        let mut a: Vec<*const f32> = act.iter().map(|r| r.as_ptr()).collect();
        let mut r: Vec<*const f32> = reward.iter().map(|r| r.as_ptr()).collect();
        let mut t: Vec<*const i8> = is_terminated.iter().map(|r| r.as_ptr()).collect();
        let mut u: Vec<*const i8> = is_truncated.iter().map(|r| r.as_ptr()).collect();
        check(unsafe {
            ffi::bdr_awac_group_push(
                self.g,
                hs.as_mut_ptr(),
                n as u64,
                o.as_mut_ptr(),
                x.as_mut_ptr(),
                std::ptr::null(),
                a.as_mut_ptr(),
                r.as_mut_ptr(),
                t.as_mut_ptr(),
                u.as_mut_ptr(),
            )
        })
    }

    /// The largest `n` one [`Self::push`] of f32 rows takes for these buffers (`bdr_awac_group_push_max_rows`).
    pub fn push_max_rows(&mut self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<usize> {
        let mut hs = self.buffer_handles(buffers)?;
        let mut n = 0u64;
        check(unsafe { ffi::bdr_awac_group_push_max_rows(self.g, hs.as_mut_ptr(), std::ptr::null(), &mut n) })?;
        Ok(n as usize)
    }

    /// `Trainer::train` (`trainer.rs:267-327`) with `Trainer::post_process` for all members in lockstep in the compiled loop
    /// `bdr_trainer_train_cgroup_post`: member `i` on `envs[i]` - the C view of an environment that writes rows of
    /// `obs_dtypes[i]` (`BDR_DTYPE_F32` / `BDR_DTYPE_F64`) and `obs_row_bytes[i]` bytes and reads one f32 action row - and
    /// `buffers[i]`; one group sample, one group push and at most one group opt per iteration.  `config.act_row_bytes` must be
    /// `4 * act_dim`.  Post-processing as [`Self::train_offline`]: with both intervals 0, `evaluators` and `model_dirs` may be empty.
    #[allow(clippy::too_many_arguments)]
    pub fn train(
        &mut self,
        envs: &[ffi::bdr_env_vtable],
        buffers: &mut [AmdReplayBuffer<O, A>],
        obs_row_bytes: &[u64],
        obs_dtypes: &[i32],
        config: &ffi::bdr_trainer_config,
        evaluators: &[ffi::bdr_evaluator],
        eval_interval: usize,
        save_interval: usize,
        model_dirs: &[&Path],
    ) -> Result<Vec<ffi::bdr_trainer_stats>> {
        let n = self.members.len();
        if envs.len() != n || obs_row_bytes.len() != n || obs_dtypes.len() != n {
            return Err(anyhow!("{} members need {} environments, row sizes and dtypes", n, n));
        }
        if (eval_interval > 0 && evaluators.len() != n) || ((eval_interval > 0 || save_interval > 0) && model_dirs.len() != n) {
            return Err(anyhow!("{} members need {} evaluators and model directories", n, n));
        }
        let mut hs = self.buffer_handles(buffers)?;
        let mut ops: ffi::bdr_cgroup_trainer_ops = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_awac_group_ctrainer_ops_default(&mut ops, self.g, hs.as_mut_ptr()) };
        let mut dirs = Vec::with_capacity(n);
        for d in model_dirs {
            dirs.push(CString::new(d.to_string_lossy().as_bytes())?);
        }
        let mut dir_ptrs: Vec<*const c_char> = dirs.iter().map(|d| d.as_ptr()).collect();
        // SAFETY: bdr_awac_group_trainer_post_default fills every field.
        let mut post: ffi::bdr_bc_group_trainer_post = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_awac_group_trainer_post_default(&mut post, self.g) };
        post.eval_interval = eval_interval as u64;
        post.save_interval = save_interval as u64;
        post.evaluators = if evaluators.is_empty() { std::ptr::null() } else { evaluators.as_ptr() };
        post.model_dirs = if dir_ptrs.is_empty() { std::ptr::null_mut() } else { dir_ptrs.as_mut_ptr() };
        let mut stats = vec![ffi::bdr_trainer_stats::default(); n];
        check(unsafe {
            ffi::bdr_trainer_train_cgroup_post(
                config,
                obs_row_bytes.as_ptr(),
                obs_dtypes.as_ptr(),
                &ops,
                envs.as_ptr(),
                &post,
                None,
                std::ptr::null_mut(),
                stats.as_mut_ptr(),
            )
        })?;
        self.sync()?;
        Ok(stats)
    }


    /// Member `dst` becomes a copy of member `src` for every `(src, dst)` of `pairs`, ONE launch whatever their number
    /// (`bdr_awac_group_copy_members`); does not synchronise.  Every arena of the model table moves (networks and targets, the last
    /// gradient, exp_avg, exp_avg_sq) with the optimizer step counters, and with `hyper` every settable hyperparameter; the
    /// destination keeps its seed, noise counter, mode, act path, buffer and index stream, n_opts and best-model bookkeeping.
    /// Refused, naming the pair, before anything moves: an index out of range, `src == dst`, a destination listed twice, a member
    /// that is a destination in one pair and a source in another.  An empty list does nothing.
    pub fn copy_members(&mut self, pairs: &[(u32, u32)], hyper: bool) -> Result<()> {
        if pairs.is_empty() {
            return Ok(());
        }
        let src: Vec<u32> = pairs.iter().map(|p| p.0).collect();
        let dst: Vec<u32> = pairs.iter().map(|p| p.1).collect();
        let flags = if hyper { ffi::BDR_COPY_HYPER } else { 0 };
        check(unsafe { ffi::bdr_awac_group_copy_members(self.g, src.as_ptr(), dst.as_ptr(), pairs.len() as u32, flags) })
    }

    /// Waits for everything the group and its members have enqueued (`bdr_awac_group_sync`).
    pub fn sync(&mut self) -> Result<()> {
        check(unsafe { ffi::bdr_awac_group_sync(self.g) })
    }
}

impl<E, O, A> Drop for AmdAwacGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    fn drop(&mut self) {
        expect(unsafe { ffi::bdr_awac_group_destroy(self.g) }, "bdr_awac_group_destroy");
        for m in self.members.iter_mut() {
            m.a.h = std::ptr::null_mut(); // destroyed with the group; bdr_agent_destroy(NULL) in the member's own drop is a no-op
        }
    }
}

/// A group of candle SAC agents of one shape whose `Agent::opt` (`Sac::opt_`, sac/base.rs:124-134) runs as the launch sequence of ONE
/// member, every launch serving all members (`bdr_candle_sac_group_*`): 3 Lp + 4 Lq + 10 launches per round for Lp, Lq layers of
/// actor and critic, whatever the number of members.  The members may differ in seed, discount, the critics' tau, critic loss, the
/// entropy mode (`Fix` or `Auto`), action limit, log-std clamps, learning rates, optimizers and train / eval mode; member `i` steps
/// on `buffers[i]`, a uniform buffer of its own or a view of one ([`AmdReplayBuffer::view`]), and pushes into it between rounds as
/// the online agent it is.  A round draws its noise inside the round: a member in train mode takes `2 * batch_size * act_dim` draws
/// at its own noise counter, the stream its own `sample` and the group's `sample` continue.
///
/// A launch grouping, not an agent kind: the members are ordinary [`AmdCandleSac`] agents ([`AmdCandleSacGroup::member_mut`]) on the
/// group's stream.  Results are bit for bit those of stepping the same agents one after the other.  Owns its members: dropping the
/// group destroys them (`bdr_candle_sac_group_destroy`).
pub struct AmdCandleSacGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    g: *mut ffi::bdr_candle_sac_group,
    members: Vec<AmdCandleSac<E, O, A>>,
}

// SAFETY: as `AgentHandle` - one HIP stream for the group and its members, all device work behind `&mut`.
unsafe impl<E: Env, O: RowBatch, A: RowBatch> Send for AmdCandleSacGroup<E, O, A> {}

impl<E, O, A> AmdCandleSacGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    /// Groups agents that already exist.  Fails, naming the first member concerned and the reason, unless all members are candle
    /// SAC agents of one shape (obs and act dims, both networks, the actor kind, at most two critics, batch size) with `n_updates_per_opt == 1`
    /// on one device; the agents are then dropped as ordinary agents.
    pub fn adopt(members: Vec<AmdCandleSac<E, O, A>>) -> Result<Self> {
        if members.is_empty() {
            return Err(anyhow!("a group needs at least one member"));
        }
        let mut hs: Vec<*const ffi::bdr_agent> = members.iter().map(|m| m.a.h as *const ffi::bdr_agent).collect();
        let mut g = std::ptr::null_mut();
        check(unsafe { ffi::bdr_candle_sac_group_create(hs.as_mut_ptr(), hs.len() as u32, &mut g) })?;
        Ok(Self { g, members })
    }

    pub fn handle(&self) -> *mut ffi::bdr_candle_sac_group {
        self.g
    }

    pub fn len(&self) -> usize {
        self.members.len()
    }

    pub fn is_empty(&self) -> bool {
        self.members.is_empty()
    }

    pub fn member(&self, i: usize) -> &AmdCandleSac<E, O, A> {
        &self.members[i]
    }

    /// A member as the ordinary agent it is (`Agent`, `Policy`, `SyncModel`, `save_params` ...).
    pub fn member_mut(&mut self, i: usize) -> &mut AmdCandleSac<E, O, A> {
        &mut self.members[i]
    }

    /// `bdr_candle_sac_group_info`: `form` is `ffi::BDR_GROUP_FORM_CANDLE_SAC_LAYERS`, `launches_per_round` the kernel launches of one update
    /// round, `kernel_launches` those the group's own calls have enqueued since it was created.
    pub fn info(&self) -> Result<ffi::bdr_group_info> {
        let mut out = ffi::bdr_group_info::default();
        check(unsafe { ffi::bdr_candle_sac_group_info(self.g, &mut out) })?;
        Ok(out)
    }

    fn buffer_handles(&self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<Vec<*const ffi::bdr_replay>> {
        if buffers.len() != self.members.len() {
            return Err(anyhow!("{} members need {} buffers, got {}", self.members.len(), self.members.len(), buffers.len()));
        }
        Ok(buffers.iter().map(|b| b.h as *const ffi::bdr_replay).collect())
    }

    /// `Agent::opt` of every member, member `i` on `buffers[i]`; only enqueues.  A refused call (a prioritized, empty, mismatched
    /// or shared buffer) leaves every member and every buffer where it was.
    pub fn opt(&mut self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<()> {
        let mut hs = self.buffer_handles(buffers)?;
        check(unsafe { ffi::bdr_candle_sac_group_opt(self.g, hs.as_mut_ptr()) })
    }

    /// `Agent::opt_with_record` of every member: the same round, one synchronisation, the members' `Record`s (the three
    /// keys of a SAC record) in member order.
    pub fn opt_with_record(&mut self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<Vec<Record>> {
        const CAP: usize = 8;
        let mut hs = self.buffer_handles(buffers)?;
        let n = self.members.len();
        let mut vals = vec![0f32; n * CAP];
        let mut counts = vec![0i32; n];
        check(unsafe { ffi::bdr_candle_sac_group_opt_with_scalars(self.g, hs.as_mut_ptr(), vals.as_mut_ptr(), CAP as i32, counts.as_mut_ptr()) })?;
        let mut out = Vec::with_capacity(n);
        for (i, m) in self.members.iter_mut().enumerate() {
            let keys = m.a.record_keys().to_vec();
            let mut record = Record::empty();
            for (k, v) in keys.iter().zip(vals[i * CAP..].iter().take(counts[i] as usize)) {
                record.insert(k.clone(), RecordValue::Scalar(*v));
            }
            out.push(record);
        }
        Ok(out)
    }

    /// `Policy::sample` of every member in ONE launch (`bdr_candle_sac_group_sample`): member `i` acts on the `n` rows of `rows[i]`
    /// (`n * obs_dim` f32 values, the same `n` for every member; two members may name the same slice) and gets `n * act_dim`
    /// actions, the bits of its own `bdr_agent_sample_raw` in its current mode at its current noise counter: a member in train mode
    /// takes `n * act_dim` draws of its noise stream, a member in eval mode none.  `norms[i]`: the normaliser of member `i`'s rows,
    /// or null; an empty slice means none for anybody.
    pub fn sample(&mut self, n: usize, rows: &[&[f32]], norms: &[*const ffi::bdr_obs_norm]) -> Result<Vec<Vec<f32>>> {
        self.sample_with(None, n, rows, norms)
    }

    /// The same for the members `members` (strictly ascending indices) only (`bdr_candle_sac_group_sample_members`).  `rows` and the result
    /// still have one entry per member; the entries of members that are not selected are not read and stay empty, and their noise
    /// counters stay where they were.
    pub fn sample_members(&mut self, members: &[u32], n: usize, rows: &[&[f32]], norms: &[*const ffi::bdr_obs_norm]) -> Result<Vec<Vec<f32>>> {
        self.sample_with(Some(members), n, rows, norms)
    }

    fn sample_with(&mut self, members: Option<&[u32]>, n: usize, rows: &[&[f32]], norms: &[*const ffi::bdr_obs_norm]) -> Result<Vec<Vec<f32>>> {
        let p = self.members.len();
        if rows.len() != p || !(norms.is_empty() || norms.len() == p) {
            return Err(anyhow!("{} members need {} row slices and {} normalisers (or none), got {} and {}", p, p, p, rows.len(), norms.len()));
        }
        let act_dim = self.members[0].act_dim();
        let selected = |i: usize| members.map_or(true, |m| m.contains(&(i as u32)));
        let mut out: Vec<Vec<f32>> = (0..p).map(|i| if selected(i) { vec![0f32; n * act_dim] } else { Vec::new() }).collect();
        for i in (0..p).filter(|&i| selected(i)) {
            if n == 0 || rows[i].is_empty() || rows[i].len() % n != 0 {
                return Err(anyhow!("member {}: {} values are not {} rows of one width", i, rows[i].len(), n));
            }
        }
        let mut row_ptrs: Vec<*const c_void> = rows.iter().map(|r| r.as_ptr() as *const c_void).collect();
        let mut out_ptrs: Vec<*const f32> = out.iter_mut().map(|v| if v.is_empty() { std::ptr::null() } else { v.as_mut_ptr() as *const f32 }).collect();
        let mut norm_ptrs: Vec<*const ffi::bdr_obs_norm> = norms.to_vec();
        let norms_arg = if norm_ptrs.is_empty() { std::ptr::null_mut() } else { norm_ptrs.as_mut_ptr() };
        let dtypes = vec![ffi::BDR_DTYPE_F32; p];
        check(match members {
            None => unsafe { ffi::bdr_candle_sac_group_sample(self.g, norms_arg, n as u64, row_ptrs.as_mut_ptr(), dtypes.as_ptr(), out_ptrs.as_mut_ptr()) },
            Some(m) => unsafe {
                ffi::bdr_candle_sac_group_sample_members(
                    self.g,
                    m.as_ptr(),
                    m.len() as u32,
                    norms_arg,
                    n as u64,
                    row_ptrs.as_mut_ptr(),
                    dtypes.as_ptr(),
                    out_ptrs.as_mut_ptr(),
                )
            },
        })?;
        Ok(out)
    }

    /// `DefaultEvaluator` of every member in lockstep (`bdr_evaluate_bc_group` behind the candle SAC's table): member `i` on `evaluators[i]` -
    /// the C view of an evaluator of this crate with `act_row_bytes = 4 * act_dim`; f32 or float64 rows and a normaliser per member
    /// are allowed - with ONE acting launch per round over the members that still have an episode open.
    pub fn evaluate(&mut self, evaluators: &[ffi::bdr_evaluator]) -> Result<Vec<EvalResult>> {
        let n = self.members.len();
        if evaluators.len() != n {
            return Err(anyhow!("{} members need {} evaluators, got {}", n, n, evaluators.len()));
        }
        // SAFETY: bdr_candle_sac_group_eval_ops_default fills every field.
        let mut ops: ffi::bdr_bc_group_eval_ops = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_candle_sac_group_eval_ops_default(&mut ops, self.g) };
        let mut out = vec![ffi::bdr_eval_result::default(); n];
        check(unsafe { ffi::bdr_evaluate_bc_group(evaluators.as_ptr(), &ops, out.as_mut_ptr()) })?;
        Ok(out.iter().map(eval_result).collect())
    }

    /// `Trainer::train_offline` with `Trainer::post_process` for the group in compiled code
    /// (`bdr_trainer_train_offline_group_post`): `config.max_opts` update rounds, member `i` on `buffers[i]`; every `eval_interval`
    /// opt steps a lockstep evaluation on `evaluators`, member `i`'s best model in `model_dirs[i]/best`, every `save_interval` opt
    /// steps every member in `model_dirs[i]/<opt_steps>`.  An interval of 0 means never; with both 0, `evaluators` and `model_dirs`
    /// may be empty.
    pub fn train_offline(
        &mut self,
        buffers: &mut [AmdReplayBuffer<O, A>],
        config: &ffi::bdr_trainer_config,
        evaluators: &[ffi::bdr_evaluator],
        eval_interval: usize,
        save_interval: usize,
        model_dirs: &[&Path],
    ) -> Result<Vec<ffi::bdr_trainer_stats>> {
        let n = self.members.len();
        if (eval_interval > 0 && evaluators.len() != n) || ((eval_interval > 0 || save_interval > 0) && model_dirs.len() != n) {
            return Err(anyhow!("{} members need {} evaluators and model directories", n, n));
        }
        let mut hs = self.buffer_handles(buffers)?;
        let mut ops: ffi::bdr_group_trainer_ops = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_candle_sac_group_trainer_ops_default(&mut ops, self.g, hs.as_mut_ptr()) };
        let mut dirs = Vec::with_capacity(n);
        for d in model_dirs {
            dirs.push(CString::new(d.to_string_lossy().as_bytes())?);
        }
        let mut dir_ptrs: Vec<*const c_char> = dirs.iter().map(|d| d.as_ptr()).collect();
        // SAFETY: bdr_candle_sac_group_trainer_post_default fills every field.
        let mut post: ffi::bdr_bc_group_trainer_post = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_candle_sac_group_trainer_post_default(&mut post, self.g) };
        post.eval_interval = eval_interval as u64;
        post.save_interval = save_interval as u64;
        post.evaluators = if evaluators.is_empty() { std::ptr::null() } else { evaluators.as_ptr() };
        post.model_dirs = if dir_ptrs.is_empty() { std::ptr::null_mut() } else { dir_ptrs.as_mut_ptr() };
        let mut stats = vec![ffi::bdr_trainer_stats::default(); n];
        check(unsafe { ffi::bdr_trainer_train_offline_group_post(config, &ops, &post, None, std::ptr::null_mut(), stats.as_mut_ptr()) })?;
        self.sync()?;
        Ok(stats)
    }

    /// `ExperienceBufferBase::push` of `n` transitions per member, member `i`'s into `buffers[i]`, in ONE launch
    /// (`bdr_candle_sac_group_push`); only enqueues.  `obs[i]` / `next_obs[i]`: `n * obs_dim` f32 values, `act[i]`: `n * act_dim`,
    /// `reward[i]`, `is_terminated[i]`, `is_truncated[i]`: `n` values.  Each ring ends up exactly as its own `push` of those rows
    /// leaves it (a push may cross the wrap).  `n` is bounded by one staging slot ([`Self::push_max_rows`]); a refused call (a
    /// view, a prioritized ring, a single-frame store, a row width other than the members', two members on one ring, too many
    /// rows) moves nothing.  float64 rows go through `ffi::bdr_candle_sac_group_push` with `BDR_DTYPE_F64`.
    #[allow(clippy::too_many_arguments)]
    pub fn push(
        &mut self,
        buffers: &mut [AmdReplayBuffer<O, A>],
        n: usize,
        obs: &[&[f32]],
        act: &[&[f32]],
        next_obs: &[&[f32]],
        reward: &[&[f32]],
        is_terminated: &[&[i8]],
        is_truncated: &[&[i8]],
    ) -> Result<()> {
        let mut hs = self.buffer_handles(buffers)?;
        let p = self.members.len();
        if obs.len() != p || act.len() != p || next_obs.len() != p || reward.len() != p || is_terminated.len() != p || is_truncated.len() != p {
            return Err(anyhow!("{} members need {} slices of every field", p, p));
        }
        let (od, ad) = (self.members[0].obs_dim(), self.members[0].act_dim());
        for i in 0..p {
            if obs[i].len() != n * od || next_obs[i].len() != n * od || act[i].len() != n * ad {
                return Err(anyhow!("member {}: {} rows need {} observation and {} action values", i, n, n * od, n * ad));
            }
            if reward[i].len() != n || is_terminated[i].len() != n || is_truncated[i].len() != n {
                return Err(anyhow!("member {}: {} rows need {} rewards and flags", i, n, n));
            }
        }
        let mut o: Vec<*const c_void> = obs.iter().map(|r| r.as_ptr() as *const c_void).collect();
        let mut x: Vec<*const c_void> = next_obs.iter().map(|r| r.as_ptr() as *const c_void).collect();
        let mut a: Vec<*const f32> = act.iter().map(|r| r.as_ptr()).collect();
        let mut r: Vec<*const f32> = reward.iter().map(|r| r.as_ptr()).collect();
        let mut t: Vec<*const i8> = is_terminated.iter().map(|r| r.as_ptr()).collect();
        let mut u: Vec<*const i8> = is_truncated.iter().map(|r| r.as_ptr()).collect();
        check(unsafe {
            ffi::bdr_candle_sac_group_push(
                self.g,
                hs.as_mut_ptr(),
                n as u64,
                o.as_mut_ptr(),
                x.as_mut_ptr(),
                std::ptr::null(),
                a.as_mut_ptr(),
                r.as_mut_ptr(),
                t.as_mut_ptr(),
                u.as_mut_ptr(),
            )
        })
    }

    /// The largest `n` one [`Self::push`] of f32 rows takes for these buffers (`bdr_candle_sac_group_push_max_rows`).
    pub fn push_max_rows(&mut self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<usize> {
        let mut hs = self.buffer_handles(buffers)?;
        let mut n = 0u64;
        check(unsafe { ffi::bdr_candle_sac_group_push_max_rows(self.g, hs.as_mut_ptr(), std::ptr::null(), &mut n) })?;
        Ok(n as usize)
    }

    /// `Trainer::train` (`trainer.rs:267-327`) with `Trainer::post_process` for all members in lockstep in the compiled loop
    /// `bdr_trainer_train_cgroup_post`: member `i` on `envs[i]` - the C view of an environment that writes rows of
    /// `obs_dtypes[i]` (`BDR_DTYPE_F32` / `BDR_DTYPE_F64`) and `obs_row_bytes[i]` bytes and reads one f32 action row - and
    /// `buffers[i]`; one group sample, one group push and at most one group opt per iteration.  `config.act_row_bytes` must be
    /// `4 * act_dim`.  Post-processing as [`Self::train_offline`]: with both intervals 0, `evaluators` and `model_dirs` may be empty.
    #[allow(clippy::too_many_arguments)]
    pub fn train(
        &mut self,
        envs: &[ffi::bdr_env_vtable],
        buffers: &mut [AmdReplayBuffer<O, A>],
        obs_row_bytes: &[u64],
        obs_dtypes: &[i32],
        config: &ffi::bdr_trainer_config,
        evaluators: &[ffi::bdr_evaluator],
        eval_interval: usize,
        save_interval: usize,
        model_dirs: &[&Path],
    ) -> Result<Vec<ffi::bdr_trainer_stats>> {
        let n = self.members.len();
        if envs.len() != n || obs_row_bytes.len() != n || obs_dtypes.len() != n {
            return Err(anyhow!("{} members need {} environments, row sizes and dtypes", n, n));
        }
        if (eval_interval > 0 && evaluators.len() != n) || ((eval_interval > 0 || save_interval > 0) && model_dirs.len() != n) {
            return Err(anyhow!("{} members need {} evaluators and model directories", n, n));
        }
        let mut hs = self.buffer_handles(buffers)?;
        let mut ops: ffi::bdr_cgroup_trainer_ops = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_candle_sac_group_ctrainer_ops_default(&mut ops, self.g, hs.as_mut_ptr()) };
        let mut dirs = Vec::with_capacity(n);
        for d in model_dirs {
            dirs.push(CString::new(d.to_string_lossy().as_bytes())?);
        }
        let mut dir_ptrs: Vec<*const c_char> = dirs.iter().map(|d| d.as_ptr()).collect();
        // SAFETY: bdr_candle_sac_group_trainer_post_default fills every field.
        let mut post: ffi::bdr_bc_group_trainer_post = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_candle_sac_group_trainer_post_default(&mut post, self.g) };
        post.eval_interval = eval_interval as u64;
        post.save_interval = save_interval as u64;
        post.evaluators = if evaluators.is_empty() { std::ptr::null() } else { evaluators.as_ptr() };
        post.model_dirs = if dir_ptrs.is_empty() { std::ptr::null_mut() } else { dir_ptrs.as_mut_ptr() };
        let mut stats = vec![ffi::bdr_trainer_stats::default(); n];
        check(unsafe {
            ffi::bdr_trainer_train_cgroup_post(
                config,
                obs_row_bytes.as_ptr(),
                obs_dtypes.as_ptr(),
                &ops,
                envs.as_ptr(),
                &post,
                None,
                std::ptr::null_mut(),
                stats.as_mut_ptr(),
            )
        })?;
        self.sync()?;
        Ok(stats)
    }


    /// Member `dst` becomes a copy of member `src` for every `(src, dst)` of `pairs`, ONE launch whatever their number
    /// (`bdr_candle_sac_group_copy_members`); does not synchronise.  Every arena of the model table moves (networks and targets, the last
    /// gradient, exp_avg, exp_avg_sq) with the optimizer step counters, and with `hyper` every settable hyperparameter; the
    /// destination keeps its seed, noise counter, mode, act path, buffer and index stream, n_opts and best-model bookkeeping.
    /// Refused, naming the pair, before anything moves: an index out of range, `src == dst`, a destination listed twice, a member
    /// that is a destination in one pair and a source in another.  An empty list does nothing.
    pub fn copy_members(&mut self, pairs: &[(u32, u32)], hyper: bool) -> Result<()> {
        if pairs.is_empty() {
            return Ok(());
        }
        let src: Vec<u32> = pairs.iter().map(|p| p.0).collect();
        let dst: Vec<u32> = pairs.iter().map(|p| p.1).collect();
        let flags = if hyper { ffi::BDR_COPY_HYPER } else { 0 };
        check(unsafe { ffi::bdr_candle_sac_group_copy_members(self.g, src.as_ptr(), dst.as_ptr(), pairs.len() as u32, flags) })
    }

    /// Waits for everything the group and its members have enqueued (`bdr_candle_sac_group_sync`).
    pub fn sync(&mut self) -> Result<()> {
        check(unsafe { ffi::bdr_candle_sac_group_sync(self.g) })
    }
}

impl<E, O, A> Drop for AmdCandleSacGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    fn drop(&mut self) {
        expect(unsafe { ffi::bdr_candle_sac_group_destroy(self.g) }, "bdr_candle_sac_group_destroy");
        for m in self.members.iter_mut() {
            m.a.h = std::ptr::null_mut(); // destroyed with the group; bdr_agent_destroy(NULL) in the member's own drop is a no-op
        }
    }
}

/// A group of candle DQN agents (`Mlp` Q-network) of one shape whose `Agent::opt` (`Dqn::opt_`, dqn/base.rs:172-189) runs as the launch
/// sequence of ONE member, every launch serving all members (`bdr_candle_dqn_group_*`): 2 L + 4 launches per round for L layers (10
/// at the dqn_cartpole shape), whatever the number of members.  The members may differ in seed, explorer, train / eval mode,
/// optimizer, learning rate, discount, tau, soft-update interval, critic loss, record verbosity and act path; member `i` steps on
/// `buffers[i]`, a uniform buffer with i64 actions of its own or a view of one ([`AmdReplayBuffer::view`]), and pushes into it between
/// rounds as the online agent it is.  Acting runs the members' networks in one launch and then each selected member's own explorer
/// on the host: one `SmallRng` stream per member across group calls, the member's own calls and rounds.
///
/// A launch grouping, not an agent kind: the members are ordinary [`AmdCandleDqn`] agents ([`AmdCandleDqnGroup::member_mut`]) on the
/// group's stream.  Results are bit for bit those of stepping the same agents one after the other.  Owns its members: dropping the
/// group destroys them (`bdr_candle_dqn_group_destroy`).  Not built: copies between members and the hyperparameter setters.
pub struct AmdCandleDqnGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    g: *mut ffi::bdr_candle_dqn_group,
    members: Vec<AmdCandleDqn<E, O, A>>,
}

// SAFETY: as `AgentHandle` - one HIP stream for the group and its members, all device work behind `&mut`.
unsafe impl<E: Env, O: RowBatch, A: RowBatch> Send for AmdCandleDqnGroup<E, O, A> {}

impl<E, O, A> AmdCandleDqnGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    /// Groups agents that already exist.  Fails, naming the first member concerned and the reason, unless all members are candle
    /// DQN agents in the Mlp form of one shape (obs dim, number of actions, the Q-network, batch size, double_dqn) with
    /// `n_updates_per_opt == 1` on one device; the agents are then dropped as ordinary agents.
    pub fn adopt(members: Vec<AmdCandleDqn<E, O, A>>) -> Result<Self> {
        if members.is_empty() {
            return Err(anyhow!("a group needs at least one member"));
        }
        let mut hs: Vec<*const ffi::bdr_agent> = members.iter().map(|m| m.a.h as *const ffi::bdr_agent).collect();
        let mut g = std::ptr::null_mut();
        check(unsafe { ffi::bdr_candle_dqn_group_create(hs.as_mut_ptr(), hs.len() as u32, &mut g) })?;
        Ok(Self { g, members })
    }

    pub fn handle(&self) -> *mut ffi::bdr_candle_dqn_group {
        self.g
    }

    pub fn len(&self) -> usize {
        self.members.len()
    }

    pub fn is_empty(&self) -> bool {
        self.members.is_empty()
    }

    pub fn member(&self, i: usize) -> &AmdCandleDqn<E, O, A> {
        &self.members[i]
    }

    /// A member as the ordinary agent it is (`Agent`, `Policy`, `SyncModel`, `save_params` ...).
    pub fn member_mut(&mut self, i: usize) -> &mut AmdCandleDqn<E, O, A> {
        &mut self.members[i]
    }

    /// `bdr_candle_dqn_group_info`: `form` is `ffi::BDR_GROUP_FORM_CANDLE_DQN_LAYERS`, `launches_per_round` the kernel launches of one
    /// update round, `kernel_launches` those the group's own calls have enqueued since it was created.
    pub fn info(&self) -> Result<ffi::bdr_group_info> {
        let mut out = ffi::bdr_group_info::default();
        check(unsafe { ffi::bdr_candle_dqn_group_info(self.g, &mut out) })?;
        Ok(out)
    }

    fn buffer_handles(&self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<Vec<*const ffi::bdr_replay>> {
        if buffers.len() != self.members.len() {
            return Err(anyhow!("{} members need {} buffers, got {}", self.members.len(), self.members.len(), buffers.len()));
        }
        Ok(buffers.iter().map(|b| b.h as *const ffi::bdr_replay).collect())
    }

    /// `Agent::opt` of every member, member `i` on `buffers[i]`; only enqueues.  A refused call (a prioritized, empty, mismatched
    /// or shared buffer) leaves every member and every buffer where it was.
    pub fn opt(&mut self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<()> {
        let mut hs = self.buffer_handles(buffers)?;
        check(unsafe { ffi::bdr_candle_dqn_group_opt(self.g, hs.as_mut_ptr()) })
    }

    /// `Agent::opt_with_record` of every member (dqn/base.rs:307-331): the same round, one synchronisation, the members' `Record`s
    /// in member order.  A member skipped for an out-of-range action is reported as "member <i>: ...".
    pub fn opt_with_record(&mut self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<Vec<Record>> {
        const CAP: usize = 128;
        let mut hs = self.buffer_handles(buffers)?;
        let n = self.members.len();
        let mut vals = vec![0f32; n * CAP];
        let mut counts = vec![0i32; n];
        check(unsafe { ffi::bdr_candle_dqn_group_opt_with_scalars(self.g, hs.as_mut_ptr(), vals.as_mut_ptr(), CAP as i32, counts.as_mut_ptr()) })?;
        let mut out = Vec::with_capacity(n);
        for (i, m) in self.members.iter_mut().enumerate() {
            let keys = m.a.record_keys().to_vec();
            let mut record = Record::empty();
            for (k, v) in keys.iter().zip(vals[i * CAP..].iter().take(counts[i] as usize)) {
                record.insert(k.clone(), RecordValue::Scalar(*v));
            }
            out.push(record);
        }
        Ok(out)
    }

    /// `Policy::sample` of every member in ONE launch (`bdr_candle_dqn_group_sample`): member `i` acts on the `n` rows of `rows[i]`
    /// (`n * obs_dim` f32 values, the same `n` for every member) and gets `n` explored i64 actions, what its own
    /// `bdr_agent_sample_raw` gives at this point of its explorer stream.  `norms[i]`: the normaliser of member `i`'s rows, or null;
    /// an empty slice means none for anybody.
    pub fn sample(&mut self, n: usize, rows: &[&[f32]], norms: &[*const ffi::bdr_obs_norm]) -> Result<Vec<Vec<i64>>> {
        self.sample_with(None, n, rows, norms)
    }

    /// The same for the members `members` (strictly ascending indices) only (`bdr_candle_dqn_group_sample_members`).  `rows` and the
    /// result still have one entry per member; the entries of members that are not selected are not read and stay empty, and those
    /// members draw nothing.
    pub fn sample_members(&mut self, members: &[u32], n: usize, rows: &[&[f32]], norms: &[*const ffi::bdr_obs_norm]) -> Result<Vec<Vec<i64>>> {
        self.sample_with(Some(members), n, rows, norms)
    }

    fn sample_with(&mut self, members: Option<&[u32]>, n: usize, rows: &[&[f32]], norms: &[*const ffi::bdr_obs_norm]) -> Result<Vec<Vec<i64>>> {
        let p = self.members.len();
        if rows.len() != p || !(norms.is_empty() || norms.len() == p) {
            return Err(anyhow!("{} members need {} row slices and {} normalisers (or none), got {} and {}", p, p, p, rows.len(), norms.len()));
        }
        let selected = |i: usize| members.map_or(true, |m| m.contains(&(i as u32)));
        let mut out: Vec<Vec<i64>> = (0..p).map(|i| if selected(i) { vec![0i64; n] } else { Vec::new() }).collect();
        for i in (0..p).filter(|&i| selected(i)) {
            if n == 0 || rows[i].is_empty() || rows[i].len() % n != 0 {
                return Err(anyhow!("member {}: {} values are not {} rows of one width", i, rows[i].len(), n));
            }
        }
        let mut row_ptrs: Vec<*const c_void> = rows.iter().map(|r| r.as_ptr() as *const c_void).collect();
        let mut out_ptrs: Vec<*const i64> = out.iter_mut().map(|v| if v.is_empty() { std::ptr::null() } else { v.as_mut_ptr() as *const i64 }).collect();
        let mut norm_ptrs: Vec<*const ffi::bdr_obs_norm> = norms.to_vec();
        let norms_arg = if norm_ptrs.is_empty() { std::ptr::null_mut() } else { norm_ptrs.as_mut_ptr() };
        let dtypes = vec![ffi::BDR_DTYPE_F32; p];
        check(match members {
            None => unsafe { ffi::bdr_candle_dqn_group_sample(self.g, norms_arg, n as u64, row_ptrs.as_mut_ptr(), dtypes.as_ptr(), out_ptrs.as_mut_ptr()) },
            Some(m) => unsafe {
                ffi::bdr_candle_dqn_group_sample_members(
                    self.g,
                    m.as_ptr(),
                    m.len() as u32,
                    norms_arg,
                    n as u64,
                    row_ptrs.as_mut_ptr(),
                    dtypes.as_ptr(),
                    out_ptrs.as_mut_ptr(),
                )
            },
        })?;
        Ok(out)
    }

    /// The action values `[n][n_actions]` the last group acting call that selected `member` brought back for it.
    pub fn last_q(&self, member: usize, n: usize) -> Result<Vec<f32>> {
        let mut q = vec![0f32; n * self.members[member].n_actions()];
        check(unsafe { ffi::bdr_candle_dqn_group_last_q(self.g, member as u32, q.as_mut_ptr(), q.len() as u64) })?;
        Ok(q)
    }

    /// `ExperienceBufferBase::push` of `n` transitions per member, member `i`'s into `buffers[i]`, in ONE launch
    /// (`bdr_candle_dqn_group_push`); only enqueues.  `obs[i]` / `next_obs[i]`: `n * obs_dim` f32 values, `act[i]`: `n` i64 indices,
    /// `reward[i]`, `is_terminated[i]`, `is_truncated[i]`: `n` values.  Each ring ends up exactly as its own `push` of those rows
    /// leaves it (a push may cross the wrap).
    #[allow(clippy::too_many_arguments)]
    pub fn push(
        &mut self,
        buffers: &mut [AmdReplayBuffer<O, A>],
        n: usize,
        obs: &[&[f32]],
        act: &[&[i64]],
        next_obs: &[&[f32]],
        reward: &[&[f32]],
        is_terminated: &[&[i8]],
        is_truncated: &[&[i8]],
    ) -> Result<()> {
        let mut hs = self.buffer_handles(buffers)?;
        let p = self.members.len();
        if obs.len() != p || act.len() != p || next_obs.len() != p || reward.len() != p || is_terminated.len() != p || is_truncated.len() != p {
            return Err(anyhow!("{} members need {} slices of every field", p, p));
        }
        for i in 0..p {
            if n == 0 || obs[i].len() % n != 0 || next_obs[i].len() != obs[i].len() || act[i].len() != n {
                return Err(anyhow!("member {}: {} rows need {} actions and as many observation as next-observation values", i, n, n));
            }
            if reward[i].len() != n || is_terminated[i].len() != n || is_truncated[i].len() != n {
                return Err(anyhow!("member {}: {} rows need {} rewards and flags", i, n, n));
            }
        }
        let mut o: Vec<*const c_void> = obs.iter().map(|r| r.as_ptr() as *const c_void).collect();
        let mut x: Vec<*const c_void> = next_obs.iter().map(|r| r.as_ptr() as *const c_void).collect();
        let mut a: Vec<*const i64> = act.iter().map(|r| r.as_ptr()).collect();
        let mut r: Vec<*const f32> = reward.iter().map(|r| r.as_ptr()).collect();
        let mut t: Vec<*const i8> = is_terminated.iter().map(|r| r.as_ptr()).collect();
        let mut u: Vec<*const i8> = is_truncated.iter().map(|r| r.as_ptr()).collect();
        check(unsafe {
            ffi::bdr_candle_dqn_group_push(
                self.g,
                hs.as_mut_ptr(),
                n as u64,
                o.as_mut_ptr(),
                x.as_mut_ptr(),
                std::ptr::null(),
                a.as_mut_ptr(),
                r.as_mut_ptr(),
                t.as_mut_ptr(),
                u.as_mut_ptr(),
            )
        })
    }

    /// The largest `n` one [`Self::push`] of f32 rows takes for these buffers (`bdr_candle_dqn_group_push_max_rows`).
    pub fn push_max_rows(&mut self, buffers: &mut [AmdReplayBuffer<O, A>]) -> Result<usize> {
        let mut hs = self.buffer_handles(buffers)?;
        let mut n = 0u64;
        check(unsafe { ffi::bdr_candle_dqn_group_push_max_rows(self.g, hs.as_mut_ptr(), std::ptr::null(), &mut n) })?;
        Ok(n as usize)
    }

    /// `DefaultEvaluator` of every member in lockstep (`bdr_evaluate_group` behind `bdr_candle_dqn_group_eval_ops_default`): member
    /// `i` on `evaluators[i]` - the C view of an evaluator with `act_row_bytes = 8` and f32 rows - with ONE acting launch per round
    /// over the members that still have an episode open.
    pub fn evaluate(&mut self, evaluators: &[ffi::bdr_evaluator]) -> Result<Vec<EvalResult>> {
        let n = self.members.len();
        if evaluators.len() != n {
            return Err(anyhow!("{} members need {} evaluators, got {}", n, n, evaluators.len()));
        }
        // SAFETY: bdr_candle_dqn_group_eval_ops_default fills every field.
        let mut ops: ffi::bdr_group_eval_ops = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_candle_dqn_group_eval_ops_default(&mut ops, self.g) };
        let mut out = vec![ffi::bdr_eval_result::default(); n];
        check(unsafe { ffi::bdr_evaluate_group(evaluators.as_ptr(), &ops, out.as_mut_ptr()) })?;
        Ok(out.iter().map(eval_result).collect())
    }

    /// `Trainer::train` (`trainer.rs:267-327`) with `Trainer::post_process` for all members in lockstep in the compiled loop
    /// `bdr_trainer_train_group_post`: member `i` on `envs[i]` - the C view of an environment that writes f32 rows of
    /// `obs_row_bytes[i]` bytes and reads one i64 action - and `buffers[i]`; one group sample, one group push and at most one group
    /// opt per iteration.  `config.act_row_bytes` must be 8.  Every `eval_interval` opt steps a lockstep evaluation on `evaluators`,
    /// member `i`'s best model in `model_dirs[i]/best` (qnet.pt, qnet_tgt.pt), every `save_interval` opt steps every member in
    /// `model_dirs[i]/<opt_steps>`; with both intervals 0, `evaluators` and `model_dirs` may be empty.
    #[allow(clippy::too_many_arguments)]
    pub fn train(
        &mut self,
        envs: &[ffi::bdr_env_vtable],
        buffers: &mut [AmdReplayBuffer<O, A>],
        obs_row_bytes: &[u64],
        config: &ffi::bdr_trainer_config,
        evaluators: &[ffi::bdr_evaluator],
        eval_interval: usize,
        save_interval: usize,
        model_dirs: &[&Path],
    ) -> Result<Vec<ffi::bdr_trainer_stats>> {
        let n = self.members.len();
        if envs.len() != n || obs_row_bytes.len() != n {
            return Err(anyhow!("{} members need {} environments and row sizes", n, n));
        }
        if (eval_interval > 0 && evaluators.len() != n) || ((eval_interval > 0 || save_interval > 0) && model_dirs.len() != n) {
            return Err(anyhow!("{} members need {} evaluators and model directories", n, n));
        }
        let mut hs = self.buffer_handles(buffers)?;
        let mut ops: ffi::bdr_group_trainer_ops = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_candle_dqn_group_trainer_ops_default(&mut ops, self.g, hs.as_mut_ptr()) };
        let mut dirs = Vec::with_capacity(n);
        for d in model_dirs {
            dirs.push(CString::new(d.to_string_lossy().as_bytes())?);
        }
        let mut dir_ptrs: Vec<*const c_char> = dirs.iter().map(|d| d.as_ptr()).collect();
        // SAFETY: bdr_candle_dqn_group_trainer_post_default fills every field.
        let mut post: ffi::bdr_group_trainer_post = unsafe { std::mem::zeroed() };
        unsafe { ffi::bdr_candle_dqn_group_trainer_post_default(&mut post, self.g) };
        post.eval_interval = eval_interval as u64;
        post.save_interval = save_interval as u64;
        post.evaluators = if evaluators.is_empty() { std::ptr::null() } else { evaluators.as_ptr() };
        post.model_dirs = if dir_ptrs.is_empty() { std::ptr::null_mut() } else { dir_ptrs.as_mut_ptr() };
        let mut stats = vec![ffi::bdr_trainer_stats::default(); n];
        check(unsafe {
            ffi::bdr_trainer_train_group_post(config, obs_row_bytes.as_ptr(), &ops, envs.as_ptr(), &post, None, std::ptr::null_mut(), stats.as_mut_ptr())
        })?;
        self.sync()?;
        Ok(stats)
    }

    /// Waits for everything the group and its members have enqueued (`bdr_candle_dqn_group_sync`); every member settles, and a
    /// member whose update was skipped for an out-of-range action is reported as "member <i>: ...".
    pub fn sync(&mut self) -> Result<()> {
        check(unsafe { ffi::bdr_candle_dqn_group_sync(self.g) })
    }
}

impl<E, O, A> Drop for AmdCandleDqnGroup<E, O, A>
where
    E: Env,
    O: RowBatch,
    A: RowBatch,
{
    fn drop(&mut self) {
        expect(unsafe { ffi::bdr_candle_dqn_group_destroy(self.g) }, "bdr_candle_dqn_group_destroy");
        for m in self.members.iter_mut() {
            m.a.h = std::ptr::null_mut(); // destroyed with the group; bdr_agent_destroy(NULL) in the member's own drop is a no-op
        }
    }
}
