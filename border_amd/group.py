"""DqnGroup: a set of small Mlp DQN agents whose Agent::opt runs as ONE launch, one workgroup per member (bdr_agent_group_*); so do
acting (`sample`) and pushing one transition per member (`push`), and `train` drives the three from a compiled online loop.
Members of one shape beyond the one-workgroup step (Mlp[256, 256] at batch 64, the reference's dqn_cartpole) form a group too: its
update round is the layer path's launch sequence of one member, each launch serving all members (`form`, `launches_per_round`).

A launch grouping, not an agent kind: the members are ordinary `Dqn` objects (every `Dqn` method keeps working on a member and
means what it meant) that the group owns - `DqnGroup.close()` closes them, `member.close()` on a live group is refused.  Results
are bit for bit those of stepping the same agents one after the other.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .awac import Awac
from .bc import Bc
from .candle_dqn import CandleDqn
from .candle_sac import CandleSac
from .dqn import Dqn, DqnConfig, record_keys
from .iql import Iql


def raise_first(evaluators, status: int) -> None:
    """Evaluator._raise over the evaluators of a group call: an environment's exception (status 99) is raised again, else the status is checked."""
    if status == 99:
        for e in evaluators:
            if e.error is not None:
                e._raise(status)
    _lib.check(status)


GROUP_FORMS = {_lib.GROUP_FORM_ONE_WORKGROUP: "one_workgroup", _lib.GROUP_FORM_LAYERS: "layers", _lib.GROUP_FORM_BC_LAYERS: "bc_layers",
               _lib.GROUP_FORM_IQL_LAYERS: "iql_layers", _lib.GROUP_FORM_AWAC_LAYERS: "awac_layers",
               _lib.GROUP_FORM_CANDLE_SAC_LAYERS: "candle_sac_layers", _lib.GROUP_FORM_CANDLE_DQN_LAYERS: "candle_dqn_layers"}


class DqnGroup:
    STAGING_DEPTH = 8   # slots of the per-step staging ring (csrc/agent_group.hpp bdr_agent_group::STEP_SLOTS)
    PUSH_STAGING_DEPTH = 8   # slots of the push staging ring (bdr_agent_group::PUSH_SLOTS)
    _TRAINER_PREFIX = "bdr_group"   # NativeTrainer.train_group: bdr_group_trainer_ops_default / bdr_group_trainer_post_default

    def obs_row_bytes(self) -> list:
        """bytes of one float32 observation row of every member (NativeTrainer.train_group)"""
        return [4 * a.config.model_config.q_config.in_dim for a in self._members]

    def __init__(self, agents, prioritized: bool = False):
        """Adopts already built `Dqn` agents: Mlp agents that all take the one-workgroup step, or - the layer form - that all have one
        shape beyond it (at most 4 layers up to 256 wide; see bdr_agent_group_create and `form`).
        `prioritized=True`: opt / opt_with_record / push / train also accept buffers built with a `PerConfig`
        (bdr_agent_group_set_prioritized); by default a prioritized buffer is refused."""
        agents = list(agents)
        hs = (C.c_void_p * len(agents))(*[a.handle for a in agents])
        g = C.c_void_p()
        _lib.check(_lib.lib().bdr_agent_group_create(hs, len(agents), C.byref(g)))
        self._g = g
        self._members = agents
        self._keys = None
        self._bound = None   # the handle array of the buffers passed last (opt() without an argument steps on them again)
        dims = {a.config.model_config.q_config.in_dim for a in agents}
        self._in_dim = dims.pop() if len(dims) == 1 else None   # one input width for all: sample / qvalues also take a [n, in_dim] array
        self._prioritized = False
        if prioritized:
            try:
                self.set_prioritized(True)
            except Exception:
                _lib.lib().bdr_agent_group_destroy(g)   # (destroys the adopted members)
                self._g = None
                for a in agents:
                    a._h = None
                raise

    @classmethod
    def build(cls, configs, prioritized: bool = False) -> "DqnGroup":
        """One `Dqn` per DqnConfig, grouped.  Nothing is left behind when a config is refused."""
        agents = []
        try:
            for c in configs:
                agents.append(Dqn.build(c))
            return cls(agents, prioritized=prioritized)
        except Exception:
            for a in agents:
                a.close()
            raise

    @property
    def members(self):
        return list(self._members)

    def __len__(self):
        return len(self._members)

    def info(self) -> dict:
        """bdr_agent_group_info: {"form": "one_workgroup" | "layers", "n_members", "launches_per_round", "kernel_launches"}."""
        i = _lib.GroupInfoC()
        _lib.check(_lib.lib().bdr_agent_group_info(self._g, C.byref(i)))
        return {"form": "layers" if i.form == _lib.GROUP_FORM_LAYERS else "one_workgroup", "n_members": i.n_members,
                "launches_per_round": i.launches_per_round, "kernel_launches": i.kernel_launches}

    @property
    def form(self) -> str:
        """"one_workgroup": every member takes the one-workgroup step, one launch per update round.  "layers": members of one shape
        beyond it (Mlp[256, 256] at batch 64 and every net down to Mlp[64, 64] past batch 64) on the layer path's launch sequence of
        one member, each launch serving all of them."""
        return self.info()["form"]

    @property
    def launches_per_round(self) -> int:
        """kernel launches of one update round on uniform rings, whatever the number of members"""
        return self.info()["launches_per_round"]

    @property
    def kernel_launches(self) -> int:
        """kernel launches the group's own calls have enqueued since it was built"""
        return self.info()["kernel_launches"]

    @property
    def prioritized(self) -> bool:
        return self._prioritized

    def set_prioritized(self, on: bool) -> None:
        """Switches prioritized replay under the group on or off (bdr_agent_group_set_prioritized): on, the prioritized members' tree
        sampling, weights and priority updates run as a fixed number of launches per round, bit for bit what their own calls give."""
        _lib.check(_lib.lib().bdr_agent_group_set_prioritized(self._g, 1 if on else 0))
        self._prioritized = bool(on)

    @property
    def handle(self):
        return self._g

    def _buffers(self, buffers):
        if buffers is None:   # the buffers of the last call (building the handle array costs ~0.2 us per member in Python)
            if self._bound is None:
                raise ValueError("opt() without buffers needs an earlier call that named them")
            return self._bound
        buffers = list(buffers)
        if len(buffers) != len(self._members):
            raise ValueError(f"{len(self._members)} members need {len(self._members)} buffers, got {len(buffers)}")
        self._bound = (C.c_void_p * len(buffers))(*[b.handle for b in buffers])
        return self._bound

    def opt(self, buffers=None) -> None:
        """Agent::opt of every member on its own buffer: n_updates_per_opt * launches_per_round launches in all (one per round in the
        one-workgroup form); does not synchronise.
        `buffers=None`: the buffers of the last opt / opt_with_record call (they must still be open)."""
        _lib.check(_lib.lib().bdr_agent_group_opt(self._g, self._buffers(buffers)))

    def opt_with_record(self, buffers=None) -> list:
        """Agent::opt_with_record of every member (one synchronisation): a list of Record dicts in member order."""
        n, cap = len(self._members), 128
        out = np.zeros((n, cap), np.float32)
        cnt = np.zeros(n, np.int32)
        _lib.check(_lib.lib().bdr_agent_group_opt_with_scalars(self._g, self._buffers(buffers), out.ctypes.data_as(C.c_void_p), cap,
                                                               cnt.ctypes.data_as(C.c_void_p)))
        if self._keys is None:
            self._keys = [record_keys(a.handle) for a in self._members]
        return [{k: float(v) for k, v in zip(self._keys[i], out[i, :cnt[i]])} for i in range(n)]

    def _rows(self, rows):
        n = len(self._members)
        if isinstance(rows, np.ndarray) and self._in_dim is not None and rows.dtype == np.float32 and rows.shape == (n, self._in_dim) \
                and rows.flags.c_contiguous:   # one array for all members: row addresses by arithmetic, no per-row objects
            ptrs = np.uint64(rows.ctypes.data) + np.arange(n, dtype=np.uint64) * np.uint64(4 * self._in_dim)
            return rows, ptrs.ctypes.data_as(C.c_void_p), ptrs
        rows = [np.ascontiguousarray(r, dtype=np.float32).reshape(-1) for r in rows]
        if len(rows) != len(self._members):
            raise ValueError(f"{len(self._members)} members need {len(self._members)} observation rows, got {len(rows)}")
        for i, (r, a) in enumerate(zip(rows, self._members)):
            want = a.config.model_config.q_config.in_dim
            if r.size != want:
                raise ValueError(f"member {i}: an observation row of {want} f32, got {r.size}")
        return rows, (C.c_void_p * len(rows))(*[r.ctypes.data for r in rows]), None

    def qvalues(self, rows) -> list:
        """qnet.forward of one observation row per member, one launch: a list of [A_i] float32 arrays."""
        rows, ptrs, _keep = self._rows(rows)
        qs = [np.empty(a.n_actions, np.float32) for a in self._members]
        outs = (C.c_void_p * len(qs))(*[q.ctypes.data for q in qs])
        _lib.check(_lib.lib().bdr_agent_group_qvalues(self._g, ptrs, outs))
        return qs

    def sample(self, rows, return_info: bool = False, members=None):
        """Policy::sample of every member on one observation row each, one launch: int64 actions [n] (and the per-member info).
        rows: one row per member, or - when every member has the same in_dim - a float32 array [n, in_dim].
        members: a strictly ascending list of member indices (bdr_agent_group_sample_members): only those act, in one launch of
        len(members) workgroups; `rows` is still one row per member and the results still have one entry per member, of which only
        the selected ones are written.  A member that is not selected is not touched: its exploration stream and counters stay."""
        rows, ptrs, _keep = self._rows(rows)
        n = len(rows)
        act = np.zeros(n, np.int64) if members is not None else np.empty(n, np.int64)
        info = (_lib.SampleInfoC * n)()
        if members is None:
            _lib.check(_lib.lib().bdr_agent_group_sample(self._g, ptrs, act.ctypes.data_as(C.c_void_p), info))
        else:
            sel = np.ascontiguousarray(members, np.uint32).reshape(-1)
            _lib.check(_lib.lib().bdr_agent_group_sample_members(self._g, sel.ctypes.data_as(C.c_void_p), sel.size, ptrs,
                                                                 act.ctypes.data_as(C.c_void_p), info))
        if return_info:
            return act, [{"eps": i.eps, "is_random": bool(i.is_random), "n_samples_act": i.n_samples_act,
                          "n_samples_best_act": i.n_samples_best_act} for i in info]
        return act

    def evaluate(self, evaluators) -> list:
        """The Evaluator of every member in lockstep (bdr_evaluate_group): member i on evaluators[i] (a border_amd.evaluator.Evaluator
        built with act_dtype=np.int64; environment, n_episodes and reference scores may differ per member), one acting launch per
        round over the members that still have an episode open.  Each EvalResult is what evaluators[i].evaluate(member i) gives;
        the members stay in the mode they are in.  An exception raised by an environment is raised again here."""
        from .evaluator import EvalResult
        evaluators = list(evaluators)
        n = len(self._members)
        if len(evaluators) != n:
            raise ValueError(f"{n} members need {n} evaluators, got {len(evaluators)}")
        evs = (_lib.EvaluatorC * n)(*[e.c_struct() for e in evaluators])
        ops = _lib.GroupEvalOps()
        _lib.lib().bdr_group_eval_ops_default(C.byref(ops), self._g)
        out = (_lib.EvalResultC * n)()
        rc = _lib.lib().bdr_evaluate_group(evs, C.byref(ops), out)
        raise_first(evaluators, rc)
        return [EvalResult(np.float32(o.score), np.float32(o.normalized) if o.has_normalized else None, o.n_steps, o.n_episodes) for o in out]

    def push(self, obs, act, next_obs, reward, is_terminated, is_truncated, buffers=None) -> None:
        """ExperienceBufferBase::push of one transition per member into the member's own buffer, one launch; does not synchronise.
        obs / next_obs: one row per member, or a float32 array [n, in_dim] when every member has the same in_dim; act [n] (or [n, 1])
        int64, reward [n] float32, the flags [n] int8.  `buffers=None`: the buffers named last (as opt())."""
        bufs = self._buffers(buffers)
        n = len(self._members)
        _o, optrs, _ko = self._rows(obs)
        _x, xptrs, _kx = self._rows(next_obs)
        act = np.ascontiguousarray(act, np.int64).reshape(-1)
        reward = np.ascontiguousarray(reward, np.float32).reshape(-1)
        term = np.ascontiguousarray(is_terminated, np.int8).reshape(-1)
        trunc = np.ascontiguousarray(is_truncated, np.int8).reshape(-1)
        for name, a in (("act", act), ("reward", reward), ("is_terminated", term), ("is_truncated", trunc)):
            if a.size != n:
                raise ValueError(f"{n} members need {n} values of {name}, got {a.size}")
        _lib.check(_lib.lib().bdr_agent_group_push(self._g, bufs, optrs, act.ctypes.data_as(C.c_void_p), xptrs, reward.ctypes.data_as(C.c_void_p),
                                                   term.ctypes.data_as(C.c_void_p), trunc.ctypes.data_as(C.c_void_p)))

    def train(self, envs, buffers, trainer_config, on_event=None, evaluators=None, eval_interval=0, save_interval=0, model_dirs=None) -> list:
        """The compiled online loop over the group (bdr_trainer_train_group): member i on envs[i] and buffers[i], one group sample,
        one group push and at most one group opt per iteration.  on_event(member, env_steps, opt_steps, event, scalars); returns one
        statistics dict per member.  evaluators / eval_interval / save_interval / model_dirs (one Evaluator and one directory per
        member): Trainer::post_process after every opt step (bdr_trainer_train_group_post) - a lockstep evaluation every
        eval_interval opt steps with an "eval" event per member, each member's best model in model_dirs[i]/best, every member in
        model_dirs[i]/<opt_steps> every save_interval opt steps."""
        from .trainer import NativeTrainer
        self._buffers(buffers)   # (opt() / push() without buffers go on with these)
        return NativeTrainer(trainer_config).train_group(envs, self, list(buffers), on_event=on_event, evaluators=evaluators,
                                                         eval_interval=eval_interval, save_interval=save_interval, model_dirs=model_dirs)

    def sync(self) -> None:
        _lib.check(_lib.lib().bdr_agent_group_sync(self._g))

    def close(self) -> None:
        if getattr(self, "_g", None):
            _lib.check(_lib.lib().bdr_agent_group_destroy(self._g))   # destroys the members
            self._g = None
            for a in self._members:
                a._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- acting, evaluation and the offline loop of a BcGroup or an IqlGroup: one implementation over the group's C prefix ------------------
def _group_norms(group, norm):
    n = len(group._members)
    if norm is None:
        return None, None
    norms = list(norm) if isinstance(norm, (list, tuple)) else [norm] * n
    if len(norms) != n:
        raise ValueError(f"{n} members need {n} normalisers (or None), got {len(norms)}")
    return (C.c_void_p * n)(*[None if x is None else x.handle for x in norms]), norms


def _group_sample(group, fn: str, rows, norm, members) -> list:
    """`fn` / `fn`_members (bdr_bc_group_sample, bdr_iql_group_sample) on one row array per member"""
    P = len(group._members)
    od, ad = group._members[0].config.obs_dim, group._members[0].config.act_dim
    if isinstance(rows, np.ndarray):
        rows = [rows] * P
    rows = list(rows)
    if len(rows) != P:
        raise ValueError(f"{P} members need {P} row arrays, got {len(rows)}")
    sel = list(range(P)) if members is None else [int(i) for i in members]
    staged, ptrs, codes, outs, n = {}, (C.c_void_p * P)(), (C.c_int32 * P)(), [None] * P, None
    for i in sel:
        if not 0 <= i < P or rows[i] is None:
            continue   # (the library refuses it, naming the member)
        r = rows[i]
        key = id(r)
        if key not in staged:   # one host array for several members stays one host pointer
            a = np.asarray(r)
            if a.dtype != np.float32:
                a = a.astype(np.float64, copy=False)
            staged[key] = np.ascontiguousarray(a).reshape(-1, od)
        a = staged[key]
        if n is None:
            n = a.shape[0]
        elif a.shape[0] != n:
            raise ValueError(f"member {i}: {a.shape[0]} rows, the members before it {n}: one n for every member")
        ptrs[i], codes[i] = a.ctypes.data, _lib.BDR_DTYPE_F32 if a.dtype == np.float32 else _lib.BDR_DTYPE_F64
        outs[i] = np.empty((n, ad), np.float32)
    n = 1 if n is None else n
    out_ptrs = (C.c_void_p * P)(*[None if o is None else o.ctypes.data for o in outs])
    norms, _keep = _group_norms(group, norm)
    if members is None:
        _lib.check(getattr(_lib.lib(), fn)(group._g, norms, n, ptrs, codes, out_ptrs))
    else:
        s = np.ascontiguousarray(sel, np.uint32).reshape(-1)
        _lib.check(getattr(_lib.lib(), fn + "_members")(group._g, s.ctypes.data_as(C.c_void_p), s.size, norms, n, ptrs, codes, out_ptrs))
    return outs


def _group_evaluate(group, prefix: str, evaluators) -> list:
    """bdr_evaluate_bc_group behind `prefix`_eval_ops_default (bdr_bc_group, bdr_iql_group)"""
    from .evaluator import EvalResult
    evaluators = list(evaluators)
    n = len(group._members)
    if len(evaluators) != n:
        raise ValueError(f"{n} members need {n} evaluators, got {len(evaluators)}")
    evs = (_lib.EvaluatorC * n)(*[e.c_struct() for e in evaluators])
    ops = _lib.BcGroupEvalOps()
    getattr(_lib.lib(), prefix + "_eval_ops_default")(C.byref(ops), group._g)
    out = (_lib.EvalResultC * n)()
    rc = _lib.lib().bdr_evaluate_bc_group(evs, C.byref(ops), out)
    raise_first(evaluators, rc)
    return [EvalResult(np.float32(o.score), np.float32(o.normalized) if o.has_normalized else None, o.n_steps, o.n_episodes) for o in out]


def _group_train_offline(group, prefix: str, record_keys, buffers, max_opts, record_interval, on_record, evaluators, eval_interval, save_interval,
                         model_dirs, on_event) -> list:
    """bdr_trainer_train_offline_group_post behind `prefix`_trainer_ops_default / _trainer_post_default; records carry record_keys"""
    from .trainer import NativeTrainer
    n = len(group._members)
    ops = _lib.GroupTrainerOps()
    getattr(_lib.lib(), prefix + "_trainer_ops_default")(C.byref(ops), group._g, group._buffers(buffers))
    c = _lib.TrainerConfigC()
    _lib.lib().bdr_trainer_config_default(C.byref(c))
    c.max_opts, c.record_agent_info_interval = int(max_opts), int(record_interval or 0)
    failure, recs = [], [None] * n

    def cb(_ctx, member, env_steps, opt_steps, event, scalars, k):
        try:
            name = NativeTrainer.EVENTS[event]
            vals = [scalars[i] for i in range(k)]
            if on_event is not None:
                on_event(member, env_steps, opt_steps, name, vals)
            if name == "opt_record":
                recs[member] = {key: float(v) for key, v in zip(record_keys, vals)}
                if member == n - 1 and on_record is not None:
                    on_record(opt_steps, list(recs))
        except BaseException as e:  # noqa: BLE001  (an exception cannot cross the C frame: raised again below)
            failure.append(e)
    obs, st = _lib.GROUP_OBSERVER_FN(cb), (_lib.TrainerStatsC * n)()
    post = _lib.BcGroupTrainerPostC()
    getattr(_lib.lib(), prefix + "_trainer_post_default")(C.byref(post), group._g)
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
    rc = _lib.lib().bdr_trainer_train_offline_group_post(C.byref(c), C.byref(ops), C.byref(post), obs, None, st)
    if failure:
        raise failure[0]
    raise_first(evaluators, rc)
    group.sync()
    return [{k: getattr(s, k) for k, _ in _lib.TrainerStatsC._fields_} for s in st]


def _group_push_arrays(group, obs, act, next_obs, reward, is_terminated, is_truncated, act_dtype=np.float32):
    """The per-member arrays of a grouped push: (n, obs, next_obs, dtype codes, act, reward, is_terminated, is_truncated), each a list
    of C-contiguous arrays in member order.  A field is one array per member (a list or tuple) or ONE ndarray that every member takes."""
    P = len(group._members)
    od, ad = group._members[0].config.obs_dim, group._members[0].config.act_dim

    def per_member(name, x):
        xs = [x] * P if isinstance(x, np.ndarray) else list(x)
        if len(xs) != P:
            raise ValueError(f"{P} members need {P} arrays of {name} (or one array for all), got {len(xs)}")
        return xs

    def rows(name, x):   # float64 stays float64, everything else becomes float32
        out, seen = [], {}
        for r in per_member(name, x):
            if id(r) not in seen:
                a = np.asarray(r)
                seen[id(r)] = np.ascontiguousarray(a, np.float64 if a.dtype == np.float64 else np.float32).reshape(-1, od)
            out.append(seen[id(r)])
        return out

    def cols(name, x, dtype, width):
        out, seen = [], {}
        for r in per_member(name, x):
            if id(r) not in seen:
                seen[id(r)] = np.ascontiguousarray(r, dtype).reshape(-1, width) if width else np.ascontiguousarray(r, dtype).reshape(-1)
            out.append(seen[id(r)])
        return out
    o, x = rows("obs", obs), rows("next_obs", next_obs)
    a, r = cols("act", act, act_dtype, ad), cols("reward", reward, np.float32, 0)   # (act_dtype: float32 rows, or the candle DQN's one int64)
    t, u = cols("is_terminated", is_terminated, np.int8, 0), cols("is_truncated", is_truncated, np.int8, 0)
    n = o[0].shape[0]
    for i in range(P):
        if o[i].dtype != x[i].dtype:
            raise ValueError(f"member {i}: obs is {o[i].dtype}, next_obs {x[i].dtype}: one dtype per member")
        for name, arr in (("obs", o[i]), ("next_obs", x[i]), ("act", a[i]), ("reward", r[i]), ("is_terminated", t[i]), ("is_truncated", u[i])):
            if arr.shape[0] != n:
                raise ValueError(f"member {i}: {arr.shape[0]} rows of {name}, member 0 has {n} rows of obs: one n for every member and field")
    codes = [_lib.BDR_DTYPE_F64 if v.dtype == np.float64 else _lib.BDR_DTYPE_F32 for v in o]
    return n, o, x, codes, a, r, t, u


def _group_push(group, prefix: str, obs, act, next_obs, reward, is_terminated, is_truncated, buffers) -> None:
    """`prefix`_push (bdr_awac_group_push, bdr_candle_sac_group_push) of n transitions per member"""
    bufs = group._buffers(buffers)
    P = len(group._members)
    n, o, x, codes, a, r, t, u = _group_push_arrays(group, obs, act, next_obs, reward, is_terminated, is_truncated)
    ptrs = lambda arrs: (C.c_void_p * P)(*[v.ctypes.data for v in arrs])
    _lib.check(getattr(_lib.lib(), prefix + "_push")(group._g, bufs, n, ptrs(o), ptrs(x), (C.c_int32 * P)(*codes), ptrs(a), ptrs(r), ptrs(t), ptrs(u)))


def _group_push_max_rows(group, prefix: str, obs_dtypes, buffers) -> int:
    bufs = group._buffers(buffers)
    P = len(group._members)
    dts = [obs_dtypes] * P if obs_dtypes is None or isinstance(obs_dtypes, (type, np.dtype, str)) else list(obs_dtypes)
    codes = (C.c_int32 * P)(*[_lib.BDR_DTYPE_F64 if d is not None and np.dtype(d) == np.float64 else _lib.BDR_DTYPE_F32 for d in dts])
    n = C.c_uint64(0)
    _lib.check(getattr(_lib.lib(), prefix + "_push_max_rows")(group._g, bufs, codes, C.byref(n)))
    return n.value


class _OnlineGroup:
    """The online half of an AwacGroup or a CandleSacGroup: the grouped push and the compiled online loop (csrc/group_core.hpp
    group_push, csrc/trainer.hip bdr_trainer_train_cgroup_post), written once; the two classes take its methods.  BcGroup and
    IqlGroup are offline kinds and do not have it."""
    PUSH_STAGING_DEPTH = 8          # slots of the push staging ring (csrc/group_core.hpp GroupCore::PUSH_SLOTS)
    PUSH_SLOT_BYTES = 64 * 1024     # ... and the bytes of one (GroupCore::PUSH_SLOT_BYTES): 80 per member plus every member's n records

    def push(self, obs, act, next_obs, reward, is_terminated, is_truncated, buffers=None) -> None:
        """ExperienceBufferBase::push of n transitions per member into the member's own buffer, ONE launch (bdr_<kind>_group_push);
        does not synchronise.  Each field is one array per member (a list) or ONE ndarray that every member takes: obs / next_obs
        [n, obs_dim] (or [obs_dim]: n = 1) - float64 arrays stay float64 and are converted on the device exactly as
        `astype(np.float32)` does, everything else becomes float32 -, act [n, act_dim] float32, reward [n] float32, the flags [n]
        int8; the same n for every member, 1 <= n <= push_max_rows().  Every ring ends up exactly as `rb.push` of the same rows as
        float32 leaves it.  `buffers=None`: the buffers named last (as opt())."""
        _group_push(self, self._PREFIX, obs, act, next_obs, reward, is_terminated, is_truncated, buffers)

    def push_max_rows(self, obs_dtypes=None, buffers=None) -> int:
        """The largest n one `push` takes for these buffers (bdr_<kind>_group_push_max_rows): the descriptors and the n records of
        every member fit one staging slot of PUSH_SLOT_BYTES.  obs_dtypes: one dtype for all members or one per member
        (np.float64 rows are staged raw and take twice the bytes); None: float32."""
        return _group_push_max_rows(self, self._PREFIX, obs_dtypes, buffers)

    def train(self, envs, buffers, trainer_config, obs_dtype=np.float32, on_event=None, evaluators=None, eval_interval=0, save_interval=0,
              model_dirs=None) -> list:
        """The compiled online loop over the group (bdr_trainer_train_cgroup_post): member i on envs[i] and buffers[i], one group
        sample, one group push and at most one group opt per iteration; member i sees exactly the calls `NativeTrainer.train` makes
        for a lone agent.  envs[i]: reset(None) -> obs[1, obs_dim], step_with_reset(act[1, act_dim] float32) -> Step.  obs_dtype:
        np.float32 or np.float64, one for all members or one per member - the environments' rows are kept in that dtype, acted on
        and pushed as they are.  on_event(member, env_steps, opt_steps, event, scalars); returns one statistics dict per member.
        evaluators / eval_interval / save_interval / model_dirs (one Evaluator and one directory per member): Trainer::post_process
        after every opt step, as `train_offline`.  An exception raised by an environment is raised again here."""
        from .trainer import NativeTrainer
        self._buffers(buffers)   # (opt() / push() without buffers go on with these)
        return NativeTrainer(trainer_config).train_cgroup(envs, self, list(buffers), obs_dtype=obs_dtype, on_event=on_event, evaluators=evaluators,
                                                          eval_interval=eval_interval, save_interval=save_interval, model_dirs=model_dirs)


class _GroupBase:
    """What every group on csrc/group_core.hpp shares (BcGroup, IqlGroup, AwacGroup, CandleSacGroup through _DenseGroup; CandleDqnGroup): a set of agents of one kind and shape whose Agent::opt runs as the launch sequence of ONE
    member, every launch serving all members (csrc/group_core.hpp through the kind's bdr_<kind>_group_* functions).  A subclass names
    the C prefix (_PREFIX), the member class (_MEMBER) and the keys of a member's Record (RECORD_KEYS)."""
    STAGING_DEPTH = 8   # slots of the per-step staging ring (csrc/group_core.hpp GroupCore::STEP_SLOTS)
    _PREFIX = _MEMBER = None
    RECORD_KEYS = ()

    def _c(self, name):
        return getattr(_lib.lib(), f"{self._PREFIX}_{name}")

    def __init__(self, agents):
        agents = list(agents)
        hs = (C.c_void_p * len(agents))(*[a.handle for a in agents])
        g = C.c_void_p()
        _lib.check(self._c("create")(hs, len(agents), C.byref(g)))
        self._g = g
        self._members = agents
        self._bound = None   # the handle array of the buffers passed last (opt() without an argument steps on them again)
        self._bound_buffers = None   # ... and the buffers themselves: kept alive, and checked to be open, while opt() may step on them

    @classmethod
    def build(cls, configs):
        """One member agent per config, grouped.  Nothing is left behind when a config is refused."""
        agents = []
        try:
            for c in configs:
                agents.append(cls._MEMBER.build(c))
            return cls(agents)
        except Exception:
            for a in agents:
                a.close()
            raise

    @property
    def members(self):
        return list(self._members)

    def __len__(self):
        return len(self._members)

    @property
    def handle(self):
        return self._g

    def info(self) -> dict:
        """bdr_<kind>_group_info: {"form": "bc_layers" / "iql_layers" / "awac_layers" / "candle_sac_layers", "n_members", "launches_per_round", "kernel_launches"}."""
        i = _lib.GroupInfoC()
        _lib.check(self._c("info")(self._g, C.byref(i)))
        return {"form": GROUP_FORMS[i.form], "n_members": i.n_members, "launches_per_round": i.launches_per_round, "kernel_launches": i.kernel_launches}

    @property
    def form(self) -> str:
        return self.info()["form"]

    @property
    def launches_per_round(self) -> int:
        """kernel launches of one update round, whatever the number of members"""
        return self.info()["launches_per_round"]

    @property
    def kernel_launches(self) -> int:
        """kernel launches the group's own calls have enqueued since it was built"""
        return self.info()["kernel_launches"]

    def _buffers(self, buffers):
        if buffers is None:
            if self._bound is None:
                raise ValueError("opt() without buffers needs an earlier call that named them")
            for i, b in enumerate(self._bound_buffers):
                if b is not None and not b.handle:
                    raise ValueError(f"member {i}: its buffer of the last call has been closed: name the buffers again")
            return self._bound
        buffers = list(buffers)
        if len(buffers) != len(self._members):
            raise ValueError(f"{len(self._members)} members need {len(self._members)} buffers, got {len(buffers)}")
        self._bound = (C.c_void_p * len(buffers))(*[None if b is None else b.handle for b in buffers])
        self._bound_buffers = buffers
        return self._bound

    def opt(self, buffers=None) -> None:
        """Agent::opt of every member on its own buffer: launches_per_round launches in all; does not synchronise.
        `buffers=None`: the buffers of the last opt / opt_with_record call (they must still be open)."""
        _lib.check(self._c("opt")(self._g, self._buffers(buffers)))

    def opt_with_record(self, buffers=None) -> list:
        """Agent::opt_with_record of every member (one synchronisation): a list of Record dicts (RECORD_KEYS) in member order."""
        n, cap = len(self._members), 8
        out = np.zeros((n, cap), np.float32)
        cnt = np.zeros(n, np.int32)
        _lib.check(self._c("opt_with_scalars")(self._g, self._buffers(buffers), out.ctypes.data_as(C.c_void_p), cap, cnt.ctypes.data_as(C.c_void_p)))
        return [{k: float(v) for k, v in zip(self.RECORD_KEYS, out[i, :cnt[i]])} for i in range(n)]

    def sample(self, rows, norm=None, members=None) -> list:
        """Policy::sample of the members in ONE launch (bdr_<kind>_group_sample): a list of float32 arrays [n, act_dim] in member
        order, each with the bits of that member's own `sample_raw(rows[i], norm[i])` on either act path.  An IQL or AWAC member acts in the
        mode it is in (`set_train`) and at its own noise counter: in train mode it takes n * act_dim draws of its noise stream, in
        eval mode none, so group calls and the member's own calls continue one stream.
        rows: one array per member - float32 or float64, [n, obs_dim] (or [obs_dim]: n = 1), the same n for every member - or ONE
        array for all members (an ensemble on one observation batch).  norm: an ObsNormalizer for all members, a list of them /
        None per member, or None.  members: a strictly ascending list of member indices (bdr_<kind>_group_sample_members): only those
        act; the result still has one entry per member and the entries of members that were not selected are None."""
        return _group_sample(self, self._PREFIX + "_sample", rows, norm, members)

    def evaluate(self, evaluators) -> list:
        """The Evaluator of every member in lockstep (bdr_evaluate_bc_group behind the kind's table): member i on evaluators[i] (a
        border_amd.evaluator.Evaluator with act_dim = the members' act_dim; environment, n_episodes, obs_dtype, normaliser and
        reference scores may differ per member), ONE acting launch per round over the members that still have an episode open.
        Each EvalResult is what evaluators[i].evaluate(member i) gives.  An exception raised by an environment is raised again here."""
        return _group_evaluate(self, self._PREFIX, evaluators)

    def sync(self) -> None:
        _lib.check(self._c("sync")(self._g))

    def close(self) -> None:
        if getattr(self, "_g", None):
            _lib.check(self._c("destroy")(self._g))   # destroys the members
            self._g = None
            for a in self._members:
                a._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DenseGroup(_GroupBase):
    """_GroupBase plus what the four float-action kinds have and the candle DQN group has not: the compiled offline loop, copies
    between members and the hyperparameters by id."""
    COPY_STAGING_DEPTH = 8   # slots of the segment ring of copy_members (csrc/group_copy.hpp GC_SLOTS)

    def train_offline(self, buffers, max_opts: int, record_interval: int = 0, on_record=None, evaluators=None, eval_interval: int = 0,
                      save_interval: int = 0, model_dirs=None, on_event=None) -> list:
        """Trainer::train_offline over the group in compiled code (bdr_trainer_train_offline_group_post): max_opts update rounds on
        `buffers`; every record_interval-th one is an opt_with_record whose records (RECORD_KEYS) go to on_record(opt_step, records).
        evaluators / eval_interval / save_interval / model_dirs (one Evaluator and one directory per member): Trainer::post_process
        after every opt step - a lockstep evaluation every eval_interval opt steps, each member's best model in model_dirs[i]/best,
        every member in model_dirs[i]/<opt_steps> every save_interval opt steps.  on_event(member, env_steps, opt_steps, event,
        scalars) sees every event ("opt", "opt_record", "eval", "cost").  Synchronised at its end; returns one statistics dict per
        member."""
        return _group_train_offline(self, self._PREFIX, self.RECORD_KEYS, buffers, max_opts, record_interval, on_record, evaluators, eval_interval,
                                    save_interval, model_dirs, on_event)

    def copy_members(self, pairs, hyper: bool = True) -> None:
        """Member dst becomes a copy of member src for every (src, dst) of `pairs`, ONE launch whatever their number
        (bdr_<kind>_group_copy_members); does not synchronise.  Every arena of the model table moves (networks and targets, the last
        gradient, exp_avg, exp_avg_sq) with the optimizer step counters, and with hyper=True every settable hyperparameter; the
        destination keeps its seed, noise counter, mode, act path, buffer and index stream, n_opts and best-model bookkeeping.
        Refused (BdrError naming the pair) before anything moves: an index out of range, src == dst, a destination listed twice, a
        member that is a destination in one pair and a source in another.  An empty list does nothing."""
        pairs = [(int(s), int(d)) for s, d in pairs]
        if not pairs:
            return
        for s, d in pairs:
            if s < 0 or d < 0:
                raise ValueError(f"pair ({s} -> {d}): a member index is not negative")
        src = np.ascontiguousarray([s for s, _ in pairs], np.uint32)
        dst = np.ascontiguousarray([d for _, d in pairs], np.uint32)
        _lib.check(self._c("copy_members")(self._g, src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p), len(pairs),
                                           _lib.BDR_COPY_HYPER if hyper else 0))

    def get_hyper(self, member: int, name) -> float:
        """`members[member].get_hyper(name)`"""
        return self._members[member].get_hyper(name)

    def set_hyper(self, member: int, name, value: float) -> None:
        """`members[member].set_hyper(name, value)`: in force from the next round"""
        self._members[member].set_hyper(name, value)


class BcGroup(_DenseGroup):
    """A set of BC agents of one shape whose Agent::opt runs as the launch sequence of ONE member, every launch serving all members
    (bdr_bc_group_*): 2L + 4 launches per round for L layers in the "general" kernel form, 2L + 2 with the MFMA head, whatever the
    number of members.  The members may differ in seed, learning rate and optimizer; their buffers are uniform buffers of their own
    or views of one (`SimpleReplayBuffer.view`), so that P members hold one copy of a dataset.  Acting (`sample`: one launch for the
    selected members), the lockstep `evaluate` and the compiled `train_offline` with post-processing serve all members at once too.

    A launch grouping, not an agent kind: the members are ordinary `Bc` objects (every `Bc` method keeps working on a member and
    means what it meant) that the group owns - `BcGroup.close()` closes them, `member.close()` on a live group is refused.  Results
    are bit for bit those of stepping the same agents one after the other."""
    _PREFIX, _MEMBER, RECORD_KEYS = "bdr_bc_group", Bc, ("loss",)


class IqlGroup(_DenseGroup):
    """A set of IQL agents of one shape whose Agent::opt (Iql::opt_, iql/base.rs:157-188) runs as the launch sequence of ONE member,
    every launch serving all members (bdr_iql_group_*): 3 (Lq + Lv) + 2 Lp + 8 launches per round for Lv, Lq, Lp layers of value,
    critic and actor, whatever the number of members.  The members may differ in seed, tau_iql, inv_lambda, exp_adv_max, gamma, the
    critics' tau, adv_softmax, critic_loss, the action limit, the log-std clamps, learning rates and optimizers; their buffers are
    uniform buffers of their own or views of one (`SimpleReplayBuffer.view`), so that P members hold one copy of a dataset.

    A launch grouping, not an agent kind: the members are ordinary `Iql` objects (every `Iql` method keeps working on a member and
    means what it meant) that the group owns - `IqlGroup.close()` closes them, `member.close()` on a live group is refused.  Results
    are bit for bit those of stepping the same agents one after the other."""
    _PREFIX, _MEMBER, RECORD_KEYS = "bdr_iql_group", Iql, ("loss_value", "loss_critic", "loss_actor")


class AwacGroup(_DenseGroup):
    """A set of AWAC agents of one shape whose Agent::opt (Awac::opt_, awac/base.rs:170-215) runs as the launch sequence of ONE member,
    every launch serving all members (bdr_awac_group_*): 3 (Lp + Lq) + 8 launches per round for Lp, Lq layers of actor and critic,
    whatever the number of members.  The members may differ in seed, inv_lambda, exp_adv_max, gamma, the critics' tau, adv_softmax,
    critic_loss, the action limit, the log-std clamps, learning rates, optimizers and train / eval mode; their buffers are uniform
    buffers of their own or views of one (`SimpleReplayBuffer.view`), so that P members hold one copy of a dataset.

    A round draws noise inside the round (act_ and next_act): each member's mode (`set_train`) is read when the round is enqueued,
    and in train mode the member takes 2 * batch_size * act_dim draws at its own noise counter - rounds, `sample` of the group and
    the member's own `sample` / `update_on_batch` continue one stream.  `push` stores n transitions per member in one launch and
    `train` runs the compiled online loop (awac_pendulum runs Trainer::train).

    A launch grouping, not an agent kind: the members are ordinary `Awac` objects (every `Awac` method keeps working on a member and
    means what it meant) that the group owns - `AwacGroup.close()` closes them, `member.close()` on a live group is refused.  Results
    are bit for bit those of stepping the same agents one after the other."""
    _PREFIX, _MEMBER = "bdr_awac_group", Awac
    RECORD_KEYS = ("loss_critic", "loss_actor", "q_tgt_abs_mean", "adv_mean", "adv_abs_mean", "logp_mean", "reward_mean", "next_q_mean")
    PUSH_STAGING_DEPTH, PUSH_SLOT_BYTES = _OnlineGroup.PUSH_STAGING_DEPTH, _OnlineGroup.PUSH_SLOT_BYTES
    push, push_max_rows, train = _OnlineGroup.push, _OnlineGroup.push_max_rows, _OnlineGroup.train   # (the online half: BcGroup and IqlGroup do not have it)


class CandleSacGroup(_DenseGroup):
    """A set of candle SAC agents of one shape whose Agent::opt (Sac::opt_, sac/base.rs:124-134) runs as the launch sequence of ONE
    member, every launch serving all members (bdr_candle_sac_group_*): 3 Lp + 4 Lq + 10 launches per round for Lp, Lq layers of actor
    and critic (31 at an Mlp2 [h, h] actor and twin [h, h] critics), whatever the number of members.  One value for all members:
    obs_dim, act_dim, both networks' units and activation_out, the actor kind (Mlp2 or Mlp3), n_critics, batch_size.  The members may
    differ in seed, gamma, the critics' tau, critic_loss, the entropy mode (Fix(alpha) or Auto(target_entropy, lr)), the action limit,
    the log-std clamps, learning rates, optimizers and train / eval mode; their buffers are uniform buffers of their own or views of
    one (`SimpleReplayBuffer.view`).

    The members are online agents: `push` stores n transitions per member in one launch and `train` runs the compiled online loop
    (a member's own `rb.push` between rounds keeps working); the ring may grow and wrap.  A round
    draws noise inside the round (a and next_a): each member's mode (`set_train`) is read when the round is enqueued, and in train
    mode the member takes 2 * batch_size * act_dim draws at its own noise counter - rounds, `sample` of the group and the member's own
    `sample` / `update_on_batch` continue one stream.

    A launch grouping, not an agent kind: the members are ordinary `CandleSac` objects (every `CandleSac` method keeps working on a
    member and means what it meant) that the group owns - `CandleSacGroup.close()` closes them, `member.close()` on a live group is
    refused.  Results are bit for bit those of stepping the same agents one after the other."""
    _PREFIX, _MEMBER = "bdr_candle_sac_group", CandleSac
    RECORD_KEYS = ("loss_critic", "loss_actor", "ent_coef")
    PUSH_STAGING_DEPTH, PUSH_SLOT_BYTES = _OnlineGroup.PUSH_STAGING_DEPTH, _OnlineGroup.PUSH_SLOT_BYTES
    push, push_max_rows, train = _OnlineGroup.push, _OnlineGroup.push_max_rows, _OnlineGroup.train   # (the online half: BcGroup and IqlGroup do not have it)


class CandleDqnGroup(_GroupBase):
    """A set of candle DQN agents (Mlp Q-network) of one shape whose Agent::opt (Dqn::opt_, dqn/base.rs:172-189) runs as the launch
    sequence of ONE member, every launch serving all members (bdr_candle_dqn_group_*): 2 L + 4 launches per round for L layers (10 at
    the dqn_cartpole shape), whatever the number of members.  One value for all members: obs_dim, n_actions, the Q-network's units and
    activation_out, batch_size, double_dqn.  The members may differ in seed, explorer and its parameters, train / eval mode, optimizer,
    learning rate, discount_factor, tau, soft_update_interval, critic_loss, record_verbose_level and act path; their buffers are
    uniform buffers with int64 actions of their own or views of one (`SimpleReplayBuffer.view`).

    The members are online agents: `sample` acts for the selected members in one launch and then runs each member's own explorer on
    the host (one SmallRng stream per member across group calls, the member's own calls and rounds), `push` stores n transitions per
    member in one launch, `evaluate` and `train` run the compiled lockstep loops.  A member whose batch holds an out-of-range action
    is skipped on the device and reported by `sync` / `opt_with_record` as "member <i>: ..."; the others step.

    A launch grouping, not an agent kind: the members are ordinary `CandleDqn` objects (every `CandleDqn` method keeps working on a
    member and means what it meant) that the group owns - `CandleDqnGroup.close()` closes them, `member.close()` on a live group is
    refused.  Results are bit for bit those of stepping the same agents one after the other.  Not built: copy_members and the
    hyperparameter setters, the AtariCnn form, n_updates_per_opt > 1."""
    _PREFIX, _MEMBER = "bdr_candle_dqn_group", CandleDqn
    _TRAINER_PREFIX = "bdr_candle_dqn_group"   # NativeTrainer.train_group: the kind's default tables
    PUSH_STAGING_DEPTH, PUSH_SLOT_BYTES = _OnlineGroup.PUSH_STAGING_DEPTH, _OnlineGroup.PUSH_SLOT_BYTES
    push_max_rows = _OnlineGroup.push_max_rows

    def obs_row_bytes(self) -> list:
        return [4 * m.config.obs_dim for m in self._members]

    def record_keys(self, member: int = 0) -> list:
        """The keys of a member's opt_with_record record (bdr_agent_record_keys)."""
        from .handle import record_keys
        return record_keys(self._members[member].handle)

    def opt_with_record(self, buffers=None) -> list:
        """Agent::opt_with_record of every member (one synchronisation): a list of Record dicts in member order - loss, at
        record_verbose_level >= 2 the four means and the parameter statistics, then ratio_best_act."""
        n = len(self._members)
        keys = [self.record_keys(i) for i in range(n)]
        cap = max(8, max(len(k) for k in keys))   # (verbosity >= 2 adds the parameter statistics)
        out = np.zeros((n, cap), np.float32)
        cnt = np.zeros(n, np.int32)
        _lib.check(self._c("opt_with_scalars")(self._g, self._buffers(buffers), out.ctypes.data_as(C.c_void_p), cap, cnt.ctypes.data_as(C.c_void_p)))
        return [{k: np.float32(v) for k, v in zip(keys[i], out[i, :cnt[i]])} for i in range(n)]

    def sample(self, rows, norm=None, members=None) -> list:
        """Policy::sample of the members in ONE launch (bdr_candle_dqn_group_sample / _sample_members): a list of int64 arrays [n] in
        member order, each what that member's own `sample_raw(rows[i], norm[i])` gives at this point of its explorer stream.  rows,
        norm and members as for the other dense groups; the entries of members that were not selected are None (they draw nothing)."""
        P = len(self._members)
        od = self._members[0].config.obs_dim
        if isinstance(rows, np.ndarray):
            rows = [rows] * P
        rows = list(rows)
        if len(rows) != P:
            raise ValueError(f"{P} members need {P} row arrays, got {len(rows)}")
        sel = list(range(P)) if members is None else [int(i) for i in members]
        staged, ptrs, codes, outs, n = {}, (C.c_void_p * P)(), (C.c_int32 * P)(), [None] * P, None
        for i in sel:
            if not 0 <= i < P or rows[i] is None:
                continue   # (the library refuses it, naming the member)
            r = rows[i]
            if id(r) not in staged:
                a = np.asarray(r)
                if a.dtype != np.float32:
                    a = a.astype(np.float64, copy=False)
                staged[id(r)] = np.ascontiguousarray(a).reshape(-1, od)
            a = staged[id(r)]
            if n is None:
                n = a.shape[0]
            elif a.shape[0] != n:
                raise ValueError(f"member {i}: {a.shape[0]} rows, the members before it {n}: one n for every member")
            ptrs[i], codes[i] = a.ctypes.data, _lib.BDR_DTYPE_F32 if a.dtype == np.float32 else _lib.BDR_DTYPE_F64
            outs[i] = np.empty(n, np.int64)
        n = 1 if n is None else n
        out_ptrs = (C.c_void_p * P)(*[None if o is None else o.ctypes.data for o in outs])
        norms, _keep = _group_norms(self, norm)
        if members is None:
            _lib.check(self._c("sample")(self._g, norms, n, ptrs, codes, out_ptrs))
        else:
            s = np.ascontiguousarray(sel, np.uint32).reshape(-1)
            _lib.check(self._c("sample_members")(self._g, s.ctypes.data_as(C.c_void_p), s.size, norms, n, ptrs, codes, out_ptrs))
        return outs

    def last_q(self, member: int, n: int) -> np.ndarray:
        """The action values [n, n_actions] the last group `sample` that selected `member` brought back for it."""
        q = np.empty((n, self._members[member].n_actions), np.float32)
        _lib.check(self._c("last_q")(self._g, int(member), q.ctypes.data_as(C.c_void_p), q.size))
        return q

    def push(self, obs, act, next_obs, reward, is_terminated, is_truncated, buffers=None) -> None:
        """ExperienceBufferBase::push of n transitions per member into the member's own buffer, ONE launch
        (bdr_candle_dqn_group_push); does not synchronise.  As `CandleSacGroup.push`, with act [n] int64 per member."""
        bufs = self._buffers(buffers)
        P = len(self._members)
        acts = [act] * P if isinstance(act, np.ndarray) else list(act)
        if len(acts) != P:
            raise ValueError(f"{P} members need {P} arrays of act (or one array for all), got {len(acts)}")
        a = [np.ascontiguousarray(v, np.int64).reshape(-1) for v in acts]
        n, o, x, codes, a, r, t, u = _group_push_arrays(self, obs, a, next_obs, reward, is_terminated, is_truncated, act_dtype=np.int64)
        ptrs = lambda arrs: (C.c_void_p * P)(*[v.ctypes.data for v in arrs])
        _lib.check(self._c("push")(self._g, bufs, n, ptrs(o), ptrs(x), (C.c_int32 * P)(*codes), ptrs(a), ptrs(r), ptrs(t), ptrs(u)))

    def evaluate(self, evaluators) -> list:
        """The Evaluator of every member in lockstep (bdr_evaluate_group behind bdr_candle_dqn_group_eval_ops_default): member i on
        evaluators[i] (an Evaluator built with act_dtype=np.int64), ONE acting launch per round over the members that still have an
        episode open.  Each EvalResult is what evaluators[i].evaluate(member i) gives; the members stay in the mode they are in."""
        from .evaluator import EvalResult
        evaluators = list(evaluators)
        n = len(self._members)
        if len(evaluators) != n:
            raise ValueError(f"{n} members need {n} evaluators, got {len(evaluators)}")
        evs = (_lib.EvaluatorC * n)(*[e.c_struct() for e in evaluators])
        ops = _lib.GroupEvalOps()
        self._c("eval_ops_default")(C.byref(ops), self._g)
        out = (_lib.EvalResultC * n)()
        rc = _lib.lib().bdr_evaluate_group(evs, C.byref(ops), out)
        raise_first(evaluators, rc)
        return [EvalResult(np.float32(o.score), np.float32(o.normalized) if o.has_normalized else None, o.n_steps, o.n_episodes) for o in out]

    def train(self, envs, buffers, trainer_config, on_event=None, evaluators=None, eval_interval=0, save_interval=0, model_dirs=None) -> list:
        """The compiled online loop over the group (bdr_trainer_train_group / _post behind the kind's tables): as `DqnGroup.train`;
        models are saved as qnet.pt / qnet_tgt.pt in model_dirs[i]/best and model_dirs[i]/<opt_steps>."""
        from .trainer import NativeTrainer
        self._buffers(buffers)   # (opt() / push() without buffers go on with these)
        return NativeTrainer(trainer_config).train_group(envs, self, list(buffers), on_event=on_event, evaluators=evaluators,
                                                         eval_interval=eval_interval, save_interval=save_interval, model_dirs=model_dirs)
