"""Host-side mirror of the opt-step loops that call the hot path.

  Trainer.train_offline   border-core/src/trainer.rs:330-384 (pre-filled buffer, back-to-back
                          Agent::opt; warmup_period = 0, opt_interval = 1) and the gating / timing
                          of Trainer::train_step (:197-228): every record_agent_info_interval-th
                          step is opt_with_record, the timer wraps opt*() only.
  Trainer.train           trainer.rs:267-327: the online loop - Sampler::sample_and_push (trainer/sampler.rs:99-144:
                          Policy::sample on the device, env step, SimpleStepProcessor, push) then train_step.
  SimpleStepProcessor     generic_replay_buffer/step_proc.rs:62-137.
  SyntheticEnv            the benchmark's stand-in environment (envs stay in the caller).
  ParamExchange           the N>1 replacement of border-async-trainer's learner->actors model
                          channel (async_trainer/base.rs:268-272): one replica per GPU, local replay
                          shard, parameter averaging every sync_interval opt steps over RCCL.
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass

import numpy as np

from . import _lib


@dataclass
class TrainerConfig:
    """border-core/src/trainer/config.rs:30-87 (fields used by the offline loop)."""
    max_opts: int = 0
    opt_interval: int = 1
    record_agent_info_interval: int = 0   # 0: never (the reference default is usize::MAX-like "0 => unset")
    record_compute_cost_interval: int = 0
    warmup_period: int = 0


@dataclass
class Step:
    """border-core/src/base/step.rs:68-92 (single-process env: every field has one row)."""
    act: np.ndarray
    obs: np.ndarray
    reward: np.ndarray          # f32 [1]
    is_terminated: np.ndarray   # i8 [1]
    is_truncated: np.ndarray    # i8 [1]
    init_obs: "np.ndarray | None" = None

    def is_done(self) -> bool:  # step.rs:136-138
        return bool(self.is_terminated[0] == 1 or self.is_truncated[0] == 1)


class SyntheticEnv:
    """Stand-in for `Env` (border-core/src/base/env.rs:45-181): i.i.d. observations from a seeded generator, rewards
    and episode ends independent of the action.  obs rows have the replay buffer's row type."""

    def __init__(self, obs_shape, obs_dtype, seed: int = 0, p_term: float = 0.02, p_trunc: float = 0.0):
        self.obs_shape, self.obs_dtype = tuple(obs_shape), np.dtype(obs_dtype)
        self.rng = np.random.default_rng(seed)
        self.p_term, self.p_trunc = p_term, p_trunc

    def _obs(self):
        if self.obs_dtype == np.uint8:
            return self.rng.integers(0, 256, (1,) + self.obs_shape, dtype=np.uint8)
        return self.rng.standard_normal((1,) + self.obs_shape).astype(self.obs_dtype)

    def reset(self, is_done=None):
        return self._obs()

    def step_with_reset(self, act) -> Step:     # env.rs:137-161: the step; on done, init_obs = reset()
        obs = self._obs()
        rew = np.array([self.rng.choice([-1.0, 0.0, 1.0], p=[0.05, 0.9, 0.05])], np.float32)
        term = np.array([1 if self.rng.random() < self.p_term else 0], np.int8)
        trunc = np.array([1 if self.rng.random() < self.p_trunc else 0], np.int8)
        st = Step(np.asarray(act), obs, rew, term, trunc)
        if st.is_done():
            st.init_obs = self.reset()
        return st


class SimpleStepProcessor:
    """generic_replay_buffer/step_proc.rs:62-137: (prev_obs, act, obs, ...) transitions; after a terminal step the
    next transition starts from init_obs."""

    def __init__(self):
        self.prev_obs = None

    def reset(self, init_obs):
        self.prev_obs = init_obs

    def process(self, step: Step):
        assert len(step.obs) == 1
        if self.prev_obs is None:
            raise RuntimeError("prev_obs is not set. Forgot to call reset()?")
        obs, self.prev_obs = self.prev_obs, step.obs
        if step.is_done():
            assert step.init_obs is not None, "Failed to unwrap init_obs"
            self.prev_obs = step.init_obs
        return obs, step.act, step.obs, step.reward, step.is_terminated, step.is_truncated


class Sampler:
    """trainer/sampler.rs:99-144."""

    def __init__(self, env, step_proc):
        self.env, self.step_processor, self.prev_obs = env, step_proc, None

    def sample_and_push(self, agent, buffer):
        if self.prev_obs is None:
            self.prev_obs = self.env.reset(None)
            self.step_processor.reset(self.prev_obs.copy())
        act = agent.sample(self.prev_obs)                       # Policy::sample on the device
        step = self.env.step_with_reset(act)
        is_done = step.is_done()
        self.prev_obs = step.init_obs.copy() if is_done else step.obs.copy()
        buffer.push(*self.step_processor.process(step))
        if is_done:
            self.step_processor.reset(self.prev_obs.copy())
        return step


class Trainer:
    def __init__(self, config: TrainerConfig):
        self.config = config
        self.env_steps = 0
        self.opt_steps = 0
        self.timer_for_opt_steps = 0.0
        self.opt_steps_counter = 0
        self.records = []
        self.evals = []                                  # (opt_steps, EvalResult) of post_process
        self.max_eval_reward = -np.finfo(np.float32).max   # f32::MIN

    def train_step(self, agent, buffer):
        """trainer.rs:197-228."""
        c = self.config
        if self.env_steps < c.warmup_period or self.env_steps % c.opt_interval != 0:
            return None, False
        t0 = time.perf_counter()
        if c.record_agent_info_interval and (self.opt_steps + 1) % c.record_agent_info_interval == 0:
            rec = agent.opt_with_record(buffer)
        else:
            agent.opt(buffer)
            rec = None
        self.opt_steps += 1
        self.timer_for_opt_steps += time.perf_counter() - t0
        self.opt_steps_counter += 1
        return rec, True

    def average_opt_time_ms(self):
        """trainer.rs:164-174 (host-side enqueue time unless the step synchronised)."""
        return 1000.0 * self.timer_for_opt_steps / max(1, self.opt_steps_counter)

    def post_process(self, agent, evaluator, eval_interval, save_interval, model_dir):
        """trainer.rs:231-264 (an interval of 0: never).  evaluator: a border_amd.evaluator.Evaluator."""
        import os
        if eval_interval and self.opt_steps % eval_interval == 0:
            agent.eval()
            res = evaluator.evaluate(agent)
            agent.train()
            self.evals.append((self.opt_steps, res))
            if res.score > self.max_eval_reward:
                self.max_eval_reward = res.score
                agent.save_params(os.path.join(model_dir, "best"))
        if save_interval and self.opt_steps % save_interval == 0:
            agent.save_params(os.path.join(model_dir, str(self.opt_steps)))

    def train(self, env, step_proc, agent, buffer, on_step=None, evaluator=None, eval_interval=0, save_interval=0, model_dir=None):
        """trainer.rs:267-327 without recorder sinks: sample_and_push, then train_step and post_process, until max_opts.
        `on_step(step, record, is_opt)` observes every iteration (tests)."""
        sampler = Sampler(env, step_proc)
        agent.train()
        self.timer_for_samples = 0.0
        while True:
            t0 = time.perf_counter()
            step = sampler.sample_and_push(agent, buffer)
            self.timer_for_samples += time.perf_counter() - t0
            self.env_steps += 1
            rec, is_opt = self.train_step(agent, buffer)
            if rec is not None:
                self.records.append((self.opt_steps, rec))
            if is_opt and (eval_interval or save_interval):
                self.post_process(agent, evaluator, eval_interval, save_interval, model_dir)
            if on_step is not None:
                on_step(step, rec, is_opt)
            if self.opt_steps == self.config.max_opts:
                return

    def train_offline(self, agent, buffer, exchange=None, evaluator=None, eval_interval=0, save_interval=0, model_dir=None):
        """trainer.rs:330-384 without recorder sinks (out of scope: SURVEY.md 2.1 #4)."""
        self.config.warmup_period = 0
        self.config.opt_interval = 1
        agent.train()
        while True:
            self.env_steps += 1
            rec, is_opt = self.train_step(agent, buffer)
            if rec is not None:
                self.records.append((self.opt_steps, rec))
            if is_opt and (eval_interval or save_interval):
                self.post_process(agent, evaluator, eval_interval, save_interval, model_dir)
            if is_opt and exchange is not None:
                exchange.after_opt(agent, self.opt_steps)
            if self.opt_steps == self.config.max_opts:
                return


class NativeTrainer:
    """The compiled driver (csrc/trainer.hip: bdr_trainer_train / bdr_trainer_train_offline) - the loops above run in C++;
    Python only supplies the environment callbacks and, optionally, an observer."""

    EVENTS = {0: "skip", 1: "opt", 2: "opt_record", 3: "cost", 4: "eval"}

    def __init__(self, config: TrainerConfig):
        self.config = config
        self.stats = None

    def _config(self, obs_row_bytes=0, act_row_bytes=0):
        c = _lib.TrainerConfigC()
        _lib.lib().bdr_trainer_config_default(C.byref(c))
        k = self.config
        c.max_opts, c.opt_interval, c.warmup_period = k.max_opts, k.opt_interval, k.warmup_period
        c.record_agent_info_interval, c.record_compute_cost_interval = k.record_agent_info_interval, k.record_compute_cost_interval
        c.obs_row_bytes, c.act_row_bytes = obs_row_bytes, act_row_bytes
        return c

    @staticmethod
    def _observer(on_event):
        def cb(_ctx, env_steps, opt_steps, event, scalars, n):
            if on_event is not None:
                on_event(env_steps, opt_steps, NativeTrainer.EVENTS[event], [scalars[i] for i in range(n)])
        return _lib.OBSERVER_FN(cb)

    def _finish(self, st):
        self.stats = {k: getattr(st, k) for k, _ in _lib.TrainerStatsC._fields_}
        return self.stats

    @staticmethod
    def _post(evaluator, eval_interval, save_interval, model_dir, save_params=None):
        """Trainer::post_process (trainer.rs:231-264) as a bdr_trainer_post, or None when nothing of it is asked for: then the
        call is exactly the one without post-processing.  evaluator: a border_amd.evaluator.Evaluator (or a ready EvaluatorC)."""
        if evaluator is None and not eval_interval and not save_interval and model_dir is None:
            return None, None
        post = _lib.TrainerPostC()
        _lib.lib().bdr_trainer_post_default(C.byref(post))
        post.eval_interval, post.save_interval = int(eval_interval or 0), int(save_interval or 0)
        ev = None
        if evaluator is not None:
            ev = evaluator if isinstance(evaluator, _lib.EvaluatorC) else evaluator.c_struct()
            post.evaluator = C.pointer(ev)
        if model_dir is not None:
            post.model_dir = str(model_dir).encode()
        if save_params is not None:
            post.save_params = save_params
        return post, (ev, save_params)

    def train_offline(self, agent, buffer, on_event=None, ops=None, evaluator=None, eval_interval=0, save_interval=0, model_dir=None, save_params=None):
        """evaluator / eval_interval / save_interval / model_dir: Trainer::post_process after every opt step (bdr_trainer_train_offline_post);
        the observer then also gets "eval" events with [score] or [score, normalized].  Leaving them out gives bdr_trainer_train_offline."""
        if ops is None:
            ops = _lib.TrainerOps()
            _lib.lib().bdr_trainer_ops_default(C.byref(ops), agent.handle, buffer.handle)
        c, st, obs = self._config(), _lib.TrainerStatsC(), self._observer(on_event)
        post, _keep = self._post(evaluator, eval_interval, save_interval, model_dir, save_params)
        if post is None:
            _lib.check(_lib.lib().bdr_trainer_train_offline(C.byref(c), C.byref(ops), obs, None, C.byref(st)))
        else:
            rc = _lib.lib().bdr_trainer_train_offline_post(C.byref(c), C.byref(ops), C.byref(post), obs, None, C.byref(st))
            (evaluator._raise if hasattr(evaluator, "_raise") else _lib.check)(rc)
        return self._finish(st)

    def train(self, env, agent, buffer, obs_shape, obs_dtype, act_row_bytes=8, on_event=None, ops=None, act_dtype=np.int64,
              evaluator=None, eval_interval=0, save_interval=0, model_dir=None, save_params=None):
        """`env` has reset(None) -> obs[1, ...] and step_with_reset(act) -> Step (as SyntheticEnv).  Continuous-action agents
        (SAC): act_row_bytes = 4 * act_dim, act_dtype = np.float32.  evaluator / eval_interval / save_interval / model_dir: as
        train_offline (bdr_trainer_train_post)."""
        obs_dtype = np.dtype(obs_dtype)
        row = int(np.prod(obs_shape)) * obs_dtype.itemsize

        def write(ptr, arr):
            C.memmove(ptr, np.ascontiguousarray(arr, obs_dtype).ctypes.data, row)

        def reset(_ctx, obs_out):
            write(obs_out, env.reset(None))
            return 0

        def step(_ctx, act, obs_out, reward, term, trunc, init_out):
            a = np.frombuffer((C.c_char * act_row_bytes).from_address(act), act_dtype).copy()
            st = env.step_with_reset(a)
            write(obs_out, st.obs)
            reward[0], term[0], trunc[0] = float(st.reward[0]), int(st.is_terminated[0]), int(st.is_truncated[0])
            if st.is_done():
                write(init_out, st.init_obs)
            return 0

        vt = _lib.EnvVtable(None, _lib.ENV_RESET_FN(reset), _lib.ENV_STEP_FN(step))
        if getattr(env, "device_obs", False):   # device-resident observations: the callbacks get device buffers (see async_trainer.env_vtable)
            from .async_trainer import env_vtable
            self._keep = []
            vt = env_vtable(env, obs_shape, obs_dtype, act_row_bytes, act_dtype, keep=self._keep)
        if ops is None:
            ops = _lib.TrainerOps()
            _lib.lib().bdr_trainer_ops_default(C.byref(ops), agent.handle, buffer.handle)
        c, st, obs = self._config(row, act_row_bytes), _lib.TrainerStatsC(), self._observer(on_event)
        post, _keep = self._post(evaluator, eval_interval, save_interval, model_dir, save_params)
        if post is None:
            _lib.check(_lib.lib().bdr_trainer_train(C.byref(c), C.byref(ops), C.byref(vt), obs, None, C.byref(st)))
        else:
            rc = _lib.lib().bdr_trainer_train_post(C.byref(c), C.byref(ops), C.byref(vt), C.byref(post), obs, None, C.byref(st))
            (evaluator._raise if hasattr(evaluator, "_raise") else _lib.check)(rc)
        return self._finish(st)

    def train_group(self, envs, group, buffers, on_event=None, evaluators=None, eval_interval=0, save_interval=0, model_dirs=None, save_member=None):
        """bdr_trainer_train_group: Trainer::train for the members of a `DqnGroup` in lockstep, member i on envs[i] (each as `train`'s
        env: reset(None) -> obs[1, in_dim], step_with_reset(act[1] int64) -> Step) and buffers[i].  One group sample, one group push
        and at most one group opt per iteration.  on_event(member, env_steps, opt_steps, event, scalars); returns (and keeps in
        .stats) one statistics dict per member.  An exception raised by an environment ends the loop and is raised again here.
        evaluators / eval_interval / save_interval / model_dirs: Trainer::post_process per member (bdr_trainer_train_group_post; one
        Evaluator with act_dtype=np.int64 and one directory per member); the observer then also gets "eval" events with [score] or
        [score, normalized].  Leaving them out gives bdr_trainer_train_group."""
        n = len(envs)
        if n != len(group) or n != len(buffers):
            raise ValueError(f"{len(group)} members need {len(group)} environments and buffers, got {n} and {len(buffers)}")
        rows, tables = group.obs_row_bytes(), group._TRAINER_PREFIX   # (DqnGroup, CandleDqnGroup: the row sizes and the kind's default tables)
        failure = []
        keep = []

        def callbacks(env, row):
            def write(ptr, arr):
                a = np.ascontiguousarray(arr, np.float32)
                if a.nbytes != row:
                    raise ValueError(f"an observation of {row} bytes, got {a.nbytes}")
                C.memmove(ptr, a.ctypes.data, row)

            def reset(_ctx, obs_out):
                try:
                    write(obs_out, env.reset(None))
                    return 0
                except Exception as e:  # noqa: BLE001  (raised again once the loop has returned)
                    failure.append(e)
                    return 1

            def step(_ctx, act, obs_out, reward, term, trunc, init_out):
                try:
                    st = env.step_with_reset(np.array([C.c_int64.from_address(act).value], np.int64))
                    write(obs_out, st.obs)
                    reward[0], term[0], trunc[0] = float(st.reward[0]), int(st.is_terminated[0]), int(st.is_truncated[0])
                    if st.is_done():
                        write(init_out, st.init_obs)
                    return 0
                except Exception as e:  # noqa: BLE001
                    failure.append(e)
                    return 1
            fns = (_lib.ENV_RESET_FN(reset), _lib.ENV_STEP_FN(step))
            keep.append(fns)
            return _lib.EnvVtable(None, fns[0], fns[1])

        vts = (_lib.EnvVtable * n)(*[callbacks(e, r) for e, r in zip(envs, rows)])
        ops = _lib.GroupTrainerOps()
        handles = (C.c_void_p * n)(*[b.handle for b in buffers])
        getattr(_lib.lib(), tables + "_trainer_ops_default")(C.byref(ops), group.handle, handles)

        def cb(_ctx, member, env_steps, opt_steps, event, scalars, k):
            if on_event is not None:
                on_event(member, env_steps, opt_steps, NativeTrainer.EVENTS[event], [scalars[i] for i in range(k)])
        c, st, obs = self._config(0, 8), (_lib.TrainerStatsC * n)(), _lib.GROUP_OBSERVER_FN(cb)
        if evaluators is None and not eval_interval and not save_interval and model_dirs is None:
            rc = _lib.lib().bdr_trainer_train_group(C.byref(c), (C.c_uint64 * n)(*rows), C.byref(ops), vts, obs, None, st)
        else:
            post = _lib.GroupTrainerPostC()
            getattr(_lib.lib(), tables + "_trainer_post_default")(C.byref(post), group.handle)
            post.eval_interval, post.save_interval = int(eval_interval or 0), int(save_interval or 0)
            evaluators = list(evaluators) if evaluators is not None else []
            if evaluators:
                if len(evaluators) != n:
                    raise ValueError(f"{n} members need {n} evaluators, got {len(evaluators)}")
                evs = (_lib.EvaluatorC * n)(*[e.c_struct() for e in evaluators])
                post.evaluators = evs
            if model_dirs is not None:
                if len(model_dirs) != n:
                    raise ValueError(f"{n} members need {n} model directories, got {len(model_dirs)}")
                dirs = (C.c_char_p * n)(*[None if d is None else str(d).encode() for d in model_dirs])
                post.model_dirs = dirs
            if save_member is not None:
                post.save_member = save_member
            rc = _lib.lib().bdr_trainer_train_group_post(C.byref(c), (C.c_uint64 * n)(*rows), C.byref(ops), vts, C.byref(post), obs, None, st)
        if failure:
            raise failure[0]
        if evaluators:
            from .group import raise_first
            raise_first(evaluators, rc)
        _lib.check(rc)
        self.stats = [{k: getattr(s, k) for k, _ in _lib.TrainerStatsC._fields_} for s in st]
        return self.stats

    def train_cgroup(self, envs, group, buffers, obs_dtype=np.float32, on_event=None, evaluators=None, eval_interval=0, save_interval=0, model_dirs=None):
        """bdr_trainer_train_cgroup_post: Trainer::train for the members of an `AwacGroup` or a `CandleSacGroup` in lockstep, member i
        on envs[i] (reset(None) -> obs[1, obs_dim], step_with_reset(act[1, act_dim] float32) -> Step) and buffers[i].  obs_dtype:
        np.float32 or np.float64, one for all members or a list per member.  Everything else as `train_group`; the evaluators are
        built with act_dim = the members' act_dim."""
        n = len(envs)
        if n != len(group) or n != len(buffers):
            raise ValueError(f"{len(group)} members need {len(group)} environments and buffers, got {n} and {len(buffers)}")
        od, ad = group.members[0].config.obs_dim, group.members[0].config.act_dim
        dts = [np.dtype(d) for d in (obs_dtype if isinstance(obs_dtype, (list, tuple)) else [obs_dtype] * n)]
        if len(dts) != n or any(d not in (np.dtype(np.float32), np.dtype(np.float64)) for d in dts):
            raise ValueError(f"obs_dtype: np.float32 or np.float64, one for all members or one per member ({n})")
        rows = [od * d.itemsize for d in dts]
        failure = []
        keep = []

        def callbacks(env, row, dt):
            def write(ptr, arr):
                a = np.ascontiguousarray(arr, dt)
                if a.nbytes != row:
                    raise ValueError(f"an observation of {row} bytes, got {a.nbytes}")
                C.memmove(ptr, a.ctypes.data, row)

            def reset(_ctx, obs_out):
                try:
                    write(obs_out, env.reset(None))
                    return 0
                except Exception as e:  # noqa: BLE001  (raised again once the loop has returned)
                    failure.append(e)
                    return 1

            def step(_ctx, act, obs_out, reward, term, trunc, init_out):
                try:
                    st = env.step_with_reset(np.frombuffer((C.c_char * (4 * ad)).from_address(act), np.float32).copy())
                    write(obs_out, st.obs)
                    reward[0], term[0], trunc[0] = float(st.reward[0]), int(st.is_terminated[0]), int(st.is_truncated[0])
                    if st.is_done():
                        write(init_out, st.init_obs)
                    return 0
                except Exception as e:  # noqa: BLE001
                    failure.append(e)
                    return 1
            fns = (_lib.ENV_RESET_FN(reset), _lib.ENV_STEP_FN(step))
            keep.append(fns)
            return _lib.EnvVtable(None, fns[0], fns[1])

        vts = (_lib.EnvVtable * n)(*[callbacks(e, r, d) for e, r, d in zip(envs, rows, dts)])
        ops = _lib.CGroupTrainerOps()
        handles = (C.c_void_p * n)(*[b.handle for b in buffers])
        getattr(_lib.lib(), group._PREFIX + "_ctrainer_ops_default")(C.byref(ops), group.handle, handles)

        def cb(_ctx, member, env_steps, opt_steps, event, scalars, k):
            if on_event is not None:
                on_event(member, env_steps, opt_steps, NativeTrainer.EVENTS[event], [scalars[i] for i in range(k)])
        c, st, obs = self._config(0, 4 * ad), (_lib.TrainerStatsC * n)(), _lib.GROUP_OBSERVER_FN(cb)
        codes = (C.c_int32 * n)(*[_lib.BDR_DTYPE_F64 if d == np.dtype(np.float64) else _lib.BDR_DTYPE_F32 for d in dts])
        post = None
        evaluators = list(evaluators) if evaluators is not None else []
        if evaluators or eval_interval or save_interval or model_dirs is not None:
            post = _lib.BcGroupTrainerPostC()
            getattr(_lib.lib(), group._PREFIX + "_trainer_post_default")(C.byref(post), group.handle)
            post.eval_interval, post.save_interval = int(eval_interval or 0), int(save_interval or 0)
            if evaluators:
                if len(evaluators) != n:
                    raise ValueError(f"{n} members need {n} evaluators, got {len(evaluators)}")
                evs = (_lib.EvaluatorC * n)(*[e.c_struct() for e in evaluators])
                post.evaluators = evs
            if model_dirs is not None:
                if len(model_dirs) != n:
                    raise ValueError(f"{n} members need {n} model directories, got {len(model_dirs)}")
                dirs = (C.c_char_p * n)(*[None if d is None else str(d).encode() for d in model_dirs])
                post.model_dirs = dirs
        rc = _lib.lib().bdr_trainer_train_cgroup_post(C.byref(c), (C.c_uint64 * n)(*rows), codes, C.byref(ops), vts,
                                                      C.byref(post) if post is not None else None, obs, None, st)
        if failure:
            raise failure[0]
        if evaluators:
            from .group import raise_first
            raise_first(evaluators, rc)
        _lib.check(rc)
        group.sync()
        self.stats = [{k: getattr(s, k) for k, _ in _lib.TrainerStatsC._fields_} for s in st]
        return self.stats


class ParamExchange:
    """Parameter averaging across one-replica-per-GPU ranks over the library's own communicator (csrc/comm.hip): ncclAllReduce on the
    flat f32 arena + 1/N scale, enqueued on the agent's stream (or, per segment, on its communication queue); no host sync.  The
    unique id is created on rank 0 and handed to the other ranks by `bcast_bytes` (a callable(bytes|None) -> bytes, e.g. a
    torch.distributed broadcast on the control plane).  There is no other data plane here: rounds 1-5 carried a host-vector
    "torch" backend for the CPU tests; those now subclass this class (tests/test_param_exchange_gloo.py) and the N ranks-on-one-GPU
    flow tests load the communicator's host-transport test build instead (libborder_amd_hostcomm.so, build.build_hostcomm_library)."""

    def __init__(self, world_size: int, rank: int, sync_interval: int, device: int = 0, bcast_bytes=None, which=("qnet",)):
        self.world_size, self.rank, self.sync_interval = world_size, rank, sync_interval
        self.which = tuple(which)
        self.device = device
        self._comm = None
        if world_size > 1:
            self._comm = self._connect(bcast_bytes)

    def _connect(self, bcast_bytes):
        L = _lib.lib()
        uid = (C.c_uint8 * _lib.BDR_UNIQUE_ID_BYTES)()
        if self.rank == 0:
            _lib.check(L.bdr_comm_get_unique_id(uid))
        raw = bcast_bytes(bytes(uid) if self.rank == 0 else None)
        uid = (C.c_uint8 * _lib.BDR_UNIQUE_ID_BYTES)(*raw)
        h = C.c_void_p()
        _lib.check(L.bdr_comm_init_rank(uid, self.world_size, self.rank, self.device, C.byref(h)))
        return h

    @classmethod
    def rccl_or_raise(cls, world_size: int, rank: int, sync_interval: int, device: int, bcast_bytes, which=("qnet",)):
        """The library's RCCL communicator on EVERY rank, or a RuntimeError on every rank: the outcome is agreed on by all
        ranks (MIN-reduce of a success flag over the torch.distributed control-plane group), so no rank is left waiting in a
        collective and no run continues on a slower data plane without saying so.  (Round 1 demoted silently to torch's RCCL
        and then to host staging; a multi-GPU measurement must not do that.)"""
        import torch
        import torch.distributed as dist
        ex, err = None, None
        try:
            ex = cls(world_size, rank, sync_interval, device, bcast_bytes, which)
        except Exception as e:  # noqa: BLE001  (reported below, on every rank)
            err = e
        ok = torch.tensor([0 if ex is None else 1], dtype=torch.int32)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok[0]) == 0:
            if ex is not None:
                ex.close()
            raise RuntimeError(f"rank {rank}: the RCCL communicator could not be initialised on every rank ({err!r})")
        return ex

    def close(self):
        if self._comm:
            _lib.lib().bdr_comm_destroy(self._comm)
            self._comm = None

    def after_opt(self, agent, opt_steps: int) -> bool:
        """Called after every opt step; averages every sync_interval-th step."""
        if self.world_size == 1 or self.sync_interval <= 0 or opt_steps % self.sync_interval != 0:
            return False
        self.average(agent)
        return True

    def average(self, agent) -> None:
        if self.world_size == 1:
            return
        for w in self.which:
            _lib.check(_lib.lib().bdr_agent_allreduce_params(agent.handle, self._comm, agent.WHICH[w]))

    def agree(self, local_ok: bool = True) -> bool:
        """MIN over ranks of local_ok: every rank calls it before a collective (bdr_learner_ops::agree); a rank that failed
        passes False once and every rank learns it instead of blocking in the next all-reduce."""
        if self.world_size == 1:
            return bool(local_ok)
        out = C.c_int32(0)
        _lib.check(_lib.lib().bdr_comm_agree(self._comm, 1 if local_ok else 0, C.byref(out)))
        return bool(out.value)

    def broadcast(self, agent, root: int = 0) -> None:
        """The faithful learner->actors sync (SyncModel::sync_model on every actor)."""
        if self.world_size == 1:
            return
        for w in self.which:
            _lib.check(_lib.lib().bdr_agent_broadcast_params(agent.handle, self._comm, agent.WHICH[w], root))


def shard_seed(base_seed: int, rank: int) -> int:
    """Replay shard g draws from its own StdRng stream: seed + rank."""
    return base_seed + rank
