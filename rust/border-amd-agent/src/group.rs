//! A group of small `Mlp` DQN agents whose `Agent::opt` runs as ONE kernel launch, one workgroup per member
//! (`bdr_agent_group_*` of `include/border_amd.h`).
//!
//! A launch grouping, not an agent kind: the members are ordinary [`AmdDqn`] agents - every trait method keeps working on a
//! member ([`AmdDqnGroup::member_mut`]) and means what it meant - that enqueue on the group's stream, so member calls and group
//! calls stay ordered and may be mixed freely.  Results are bit for bit those of stepping the same agents one after the other.
use crate::{
    bytes::RowBatch,
    config::DqnConfig,
    dqn::AmdDqn,
    error::{check, expect},
    ffi,
    replay::AmdReplayBuffer,
};
use anyhow::{anyhow, Result};
use border_core::{
    record::{Record, RecordValue},
    Configurable, Env,
};
use std::os::raw::c_void;

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

    /// Blocks until the group's stream is idle; device-side errors of any member surface here.
    pub fn sync(&mut self) -> Result<()> {
        check(unsafe { ffi::bdr_agent_group_sync(self.g) })
    }
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
