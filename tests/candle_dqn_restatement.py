"""Independent restatement of border-candle-agent's Dqn (dqn/{base,config,explorer,model}.rs) with an Mlp Q-network: the checker of
the HIP candle DQN agent (csrc/candle_dqn.hip).  Nothing under border_amd/ imports this file.

  CandleDqnRestatement   update_critic (dqn/base.rs:59-170) and opt_'s bookkeeping (:172-190) in PyTorch autograd on the CPU; float32,
                         or float64 for the error figures (f32_f64_figures).  The network and optimizer pieces are those of
                         tests/iql_restatement.py.
  SmallRng               rand 0.8.5's SmallRng as Dqn uses it, in Python integers and numpy float32 scalars: the ONE numpy statement
                         of the contract that csrc/candle_dqn.hip's SmallRng struct states on the host.  Unpinned: nothing here can run
                         rand; tools/upstream_kat prints the vectors that would pin it.
  CandleDqnExplorer      Policy::sample's host part (dqn/base.rs:202-230, explorer.rs) on given Q rows.

update_critic:  pred = Q(obs)[act];  q = Q_tgt(next_obs)[argmax Q(next_obs)] (double_dqn: ONLINE net, first maximum) or
max_j Q_tgt(next_obs)[j];  tgt = reward + (((1 - is_terminated) * f32(gamma)) * q);  loss = mse | smooth_l1;  is_truncated,
clip_reward and clip_td_err are read by nothing.  opt_: n_updates_per_opt updates, then soft_update_counter counts OPTS and at
soft_update_interval runs track(tau): dst = f32(tau) * src + f32(1 - tau) * dst.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np
import torch

from iql_restatement import AdamState, Mlp, init_flat, mlp_count, smooth_l1  # noqa: F401

RECORD_KEYS = ("loss", "pred_mean", "reward_mean", "tgt_mean", "tgt_minus_pred_mean")
M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ the update
@dataclass
class CandleDqnSpec:
    obs_dim: int
    n_actions: int
    units: Sequence[int] = (256, 256)
    relu_out: bool = False
    lr: float = 1e-3
    adamw: Optional[dict] = field(default_factory=dict)   # AdamW kwargs (beta1, beta2, eps, wd); None: candle-optimisers' Adam
    gamma: float = 0.99
    tau: float = 0.005
    soft_update_interval: int = 1
    n_updates_per_opt: int = 1
    double_dqn: bool = False
    critic_loss: str = "Mse"

    def count(self) -> int:
        return mlp_count(self.obs_dim, self.units, self.n_actions)

    def init_params(self, seed: int):
        """(qnet, qnet_tgt) in the reference layout; the target differs from the online net, as it does after the first updates"""
        rng = np.random.default_rng(seed)
        return init_flat(self.obs_dim, self.units, self.n_actions, rng), init_flat(self.obs_dim, self.units, self.n_actions, rng)

    def to_config(self, B, batch_size: int, **kw):
        """the border_amd.CandleDqnConfig of this spec"""
        opt = B.OptimizerConfig.Adam(self.lr) if self.adamw is None else B.OptimizerConfig.AdamW(self.lr, **self.adamw)
        return B.CandleDqnConfig(
            obs_dim=self.obs_dim, n_actions=self.n_actions,
            model_config=B.CandleDqnModelConfig(B.CandleMlpConfig(tuple(self.units), "ReLU" if self.relu_out else "None"), opt),
            soft_update_interval=self.soft_update_interval, n_updates_per_opt=self.n_updates_per_opt, batch_size=batch_size,
            discount_factor=self.gamma, tau=self.tau, double_dqn=self.double_dqn, critic_loss=self.critic_loss, **kw)


def make_batch(spec: CandleDqnSpec, n: int, seed: int, p_done: float = 0.2):
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((n, spec.obs_dim)).astype(np.float32)
    next_obs = rng.standard_normal((n, spec.obs_dim)).astype(np.float32)
    act = rng.integers(0, spec.n_actions, n).astype(np.int64)
    reward = rng.standard_normal(n).astype(np.float32)
    term = (rng.random(n) < p_done).astype(np.int8)
    trunc = (rng.random(n) < p_done).astype(np.int8)
    return obs, act, next_obs, reward, term, trunc


def _cast(net: Mlp, dtype):
    net.params = [p.detach().to(dtype).requires_grad_() for p in net.params]
    return net


def _flat(params, grad=False) -> np.ndarray:
    return np.concatenate([(p.grad if grad else p).detach().numpy().reshape(-1) for p in params])


class CandleDqnRestatement:
    def __init__(self, spec: CandleDqnSpec, qnet, qnet_tgt, dtype=torch.float32):
        s = self.spec = spec
        self.dtype = dtype
        self.qnet = _cast(Mlp(s.obs_dim, s.units, s.n_actions, s.relu_out, np.asarray(qnet, np.float32)), dtype)
        self.qnet_tgt = _cast(Mlp(s.obs_dim, s.units, s.n_actions, s.relu_out, np.asarray(qnet_tgt, np.float32)), dtype)
        self.opt = AdamState(self.qnet.params, s.lr, adamw=s.adamw is not None, **(s.adamw or {}))
        self.soft_update_counter = 0
        self.n_opts = 0

    def q_next_online(self, next_obs) -> np.ndarray:
        """Q(next_obs) of the ONLINE net: the rows a double-DQN test checks for near-ties"""
        with torch.no_grad():
            return self.qnet.forward(torch.as_tensor(np.asarray(next_obs, np.float32)).to(self.dtype)).numpy()

    def qvalues(self, obs) -> np.ndarray:
        return self.q_next_online(obs)

    def update_critic(self, obs, act, next_obs, reward, is_terminated, is_truncated=None) -> dict:
        s = self.spec
        t = lambda x: torch.as_tensor(np.asarray(x, np.float32)).to(self.dtype)
        obs, next_obs, reward = t(obs), t(next_obs), t(reward).reshape(-1)
        act = torch.as_tensor(np.asarray(act, np.int64)).reshape(-1, 1)
        nt = t(np.float32(1) - np.asarray(is_terminated, np.int8).astype(np.float32))   # (1 - v) as f32; is_truncated: unread (:62)
        for p in self.qnet.params:
            p.grad = None
        pred = self.qnet.forward(obs).gather(1, act).squeeze(1)
        pred.retain_grad()
        with torch.no_grad():
            xt = self.qnet_tgt.forward(next_obs)
            y = (self.qnet.forward(next_obs) if s.double_dqn else xt).argmax(1, keepdim=True)   # torch's argmax: the first maximum
            q = xt.gather(1, y).squeeze(1)
            gamma = torch.tensor(np.float32(s.gamma)).to(self.dtype)   # `is_not_terminated * self.discount_factor`: an f32 scalar
            tgt = reward + ((nt * gamma) * q)
        loss = ((pred - tgt) ** 2).mean() if s.critic_loss == "Mse" else smooth_l1(pred, tgt)
        loss.backward()
        self.probes = dict(pred=pred.detach().numpy().copy(), q_next=q.numpy().copy(), y=y.squeeze(1).numpy().copy(), tgt=tgt.numpy().copy(),
                           dpred=pred.grad.numpy().copy(), grad=_flat(self.qnet.params, True))
        self.opt.step()
        return dict(loss=float(loss.detach()), pred_mean=float(pred.detach().mean()), reward_mean=float(reward.mean()),
                    tgt_mean=float(tgt.mean()), tgt_minus_pred_mean=float((tgt - pred.detach()).mean()))

    def opt_(self, batches) -> dict:
        """one Dqn::opt_ (:172-190) over n_updates_per_opt batches: the LAST update's record (Record::merge), then the soft update
        when the counter of opts reaches the interval"""
        s = self.spec
        assert len(batches) == s.n_updates_per_opt
        rec = {}
        for b in batches:
            rec = self.update_critic(*b)
        self.soft_update_counter += 1
        if self.soft_update_counter == s.soft_update_interval:
            self.soft_update_counter = 0
            self.track(s.tau)
        self.n_opts += 1
        return rec

    def update(self, *batch) -> dict:
        """an opt_ with one update (n_updates_per_opt == 1): what bdr_candle_dqn_update_on_batch runs"""
        return self.opt_([batch])

    def track(self, tau: float):
        f = (lambda x: torch.tensor(np.float32(x))) if self.dtype == torch.float32 else (lambda x: torch.tensor(float(x), dtype=self.dtype))
        with torch.no_grad():   # util.rs:34-49: dest = tau * src + (1 - tau) * dest, both factors cast to the tensors' dtype
            for p, tp in zip(self.qnet.params, self.qnet_tgt.params):
                tp.copy_(f(tau) * p + f(1.0 - tau) * tp)

    def params(self, name: str = "qnet") -> np.ndarray:
        if name == "qnet":
            return _flat(self.qnet.params)
        if name == "qnet_tgt":
            return _flat(self.qnet_tgt.params)
        if name == "exp_avg":
            return _flat(self.opt.m)
        if name == "exp_avg_sq":
            return _flat(self.opt.v)
        raise KeyError(name)

    def param_stats(self) -> dict:
        """util.rs param_stats: <var>_mean, <var>_std (population) of every qnet variable"""
        out = {}
        for k in range(len(self.qnet.params) // 2):
            for name, p in (("weight", self.qnet.params[2 * k]), ("bias", self.qnet.params[2 * k + 1])):
                v = p.detach().numpy().astype(np.float64)
                out[f"mlp.ln{k}.{name}_mean"] = float(v.mean())
                out[f"mlp.ln{k}.{name}_std"] = float(v.std())
        return out


def rel(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


FIGURE_KEYS = ("pred", "q_next", "tgt", "dpred", "grad", "qnet", "qnet_tgt")


def f32_f64_figures(r32: CandleDqnRestatement, r64: CandleDqnRestatement) -> dict:
    """After the same update on a float32 and a float64 restatement: how far float32 arithmetic alone moves each compared quantity.
    Max-relative for probes, gradients and the target parameters (`qnet_tgt`), max-absolute for the parameters (`qnet`)."""
    p, q = r32.probes, r64.probes
    out = {k: rel(p[k], q[k]) for k in ("pred", "q_next", "tgt", "dpred", "grad")}
    out["qnet"] = float(np.abs(r32.params("qnet") - r64.params("qnet")).max())
    out["qnet_tgt"] = rel(r32.params("qnet_tgt"), r64.params("qnet_tgt"))
    return out


def double_dqn_gap(r: CandleDqnRestatement, next_obs) -> float:
    """min over rows of (largest - second largest online Q(next_obs)) / largest |Q|: a free-running double-DQN case is meaningful
    only when no row's argmax hangs on float32 round-off"""
    q = r.q_next_online(next_obs).astype(np.float64)
    if q.shape[1] < 2:
        return math.inf
    top = np.sort(q, axis=1)[:, -2:]
    return float((top[:, 1] - top[:, 0]).min() / max(np.abs(q).max(), 1e-30))


# ------------------------------------------------------------------------------------------------ the SmallRng contract
def seed_bytes_from_u64(state: int) -> bytes:
    """rule 2: rand_core 0.6's default SeedableRng::seed_from_u64 - a PCG32 stream fills the 32 seed bytes, 4 at a time"""
    out = b""
    for _ in range(8):
        state = (state * 6364136223846793005 + 11634580027462260723) & M64
        xorshifted = (((state >> 18) ^ state) >> 27) & 0xFFFFFFFF
        rot = state >> 59
        x = ((xorshifted >> rot) | (xorshifted << ((32 - rot) & 31))) & 0xFFFFFFFF
        out += x.to_bytes(4, "little")
    return out


def _rotl(x: int, k: int) -> int:
    return ((x << k) | (x >> (64 - k))) & M64


def clz64(x: int) -> int:
    return 64 - x.bit_length()


def range_zone(A: int) -> int:
    """rule 6: UniformInt<i64>::sample_single's rejection zone for the range 0..A"""
    return ((A << clz64(A)) & M64) - 1


F32 = np.float32
MAX_RAND = F32(1.0) - F32(2.0 ** -23)


def uniform_scale(total) -> np.float32:
    """rule 7: UniformFloat<f32>::new(0, total): scale = total, stepped one ulp down while scale * (1 - 2^-23) >= total"""
    scale = F32(total)
    while F32(scale * MAX_RAND) >= F32(total):
        scale = np.frombuffer((int(np.array(scale).view(np.uint32)) - 1).to_bytes(4, "little"), np.float32)[0]
    return scale


def cumulative_weights(w):
    """rule 7: (cumulative weights of all but the last weight, total) as running f32 sums; raises ValueError where WeightedIndex::new
    errs (a weight that is not >= 0, a total of 0)"""
    w = np.asarray(w, np.float32)
    if not (w[0] >= 0):
        raise ValueError("InvalidWeight")
    total, cum = F32(w[0]), []
    for x in w[1:]:
        if not (x >= 0):
            raise ValueError("InvalidWeight")
        cum.append(total)
        total = F32(total + x)
    if total == 0:
        raise ValueError("AllWeightsZero")
    return np.asarray(cum, np.float32), total


def weighted_pick(cum, chosen) -> int:
    """the number of cumulative weights <= chosen (partition_point)"""
    return int(np.searchsorted(np.asarray(cum, np.float32), F32(chosen), side="right"))


def softmax_row(q) -> np.ndarray:
    """rule 8, in f32: e_j = exp(q_j - max), s = the sum of e_j in index order, p_j = e_j / s"""
    q = np.asarray(q, np.float32)
    e = np.exp(q - q.max(), dtype=np.float32)
    s = F32(0)
    for x in e:
        s = F32(s + x)
    return (e / s).astype(np.float32)


class SmallRng:
    def __init__(self, state):
        self.s = [int(x) for x in state]

    @classmethod
    def from_seed(cls, seed: bytes) -> "SmallRng":
        """rule 1: 32 seed bytes read as four little-endian u64"""
        assert len(seed) == 32
        return cls([int.from_bytes(seed[8 * i:8 * i + 8], "little") for i in range(4)])

    @classmethod
    def seed_from_u64(cls, seed: int) -> "SmallRng":
        return cls.from_seed(seed_bytes_from_u64(seed))

    def next_u64(self) -> int:
        """rule 3: xoshiro256++ 1.0"""
        s = self.s
        r = (_rotl((s[0] + s[3]) & M64, 23) + s[0]) & M64
        t = (s[1] << 17) & M64
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]
        s[2] ^= t
        s[3] = _rotl(s[3], 45)
        return r

    def next_u32(self) -> int:
        return self.next_u64() >> 32                                   # rule 4

    def gen_f32(self) -> np.float32:
        return F32(F32(self.next_u32() >> 8) * F32(2.0 ** -24))        # rule 5

    def gen_range(self, A: int) -> int:
        zone = range_zone(A)                                           # rule 6
        while True:
            m = self.next_u64() * A
            if (m & M64) <= zone:
                return m >> 64

    def weighted_index(self, w, detail: bool = False):
        cum, total = cumulative_weights(w)                             # rule 7
        scale = uniform_scale(total)
        u = F32(F32(self.next_u32() >> 9) * F32(2.0 ** -23))
        chosen = F32(u * scale)
        k = weighted_pick(cum, chosen)
        return (k, cum, total, chosen) if detail else k


KAT_WEIGHTS = (0.125, 0.25, 0.0625, 0.5, 0.0625)   # the weight list of tools/upstream_kat's `small_rng` section


def small_rng_kat(seed: int = 42) -> dict:
    """The `small_rng` section of tools/upstream_kat's output as THIS restatement computes it, key for key, each vector from a fresh
    generator: put beside the program's JSON, every key must be equal.  `python tests/candle_dqn_restatement.py` prints it."""
    fresh = lambda: SmallRng.seed_from_u64(seed)
    r = fresh(); u64s = [r.next_u64() for _ in range(8)]
    r = fresh(); f32_bits = [int(np.array(r.gen_f32()).view(np.uint32)) for _ in range(4)]
    r = fresh(); ranges = [r.gen_range(6) for _ in range(4)]
    r = fresh(); picks = [r.weighted_index(KAT_WEIGHTS) for _ in range(4)]
    r = fresh(); mods = [r.next_u64() % 6 for _ in range(4)]
    return {"seed": seed, "next_u64": u64s, "gen_f32_bits": f32_bits, "gen_range_0_6_i64": ranges, "weights_f32": list(KAT_WEIGHTS),
            "weighted_index": picks, "gen_u64_mod_6": mods}


class CandleDqnExplorer:
    """Policy::sample's host part on given Q rows [n][A].  kind: "softmax" | "eps_greedy"."""

    def __init__(self, kind="softmax", eps_start=1.0, eps_final=0.02, final_step=100_000, n_opts=0, seed=42, verbose_level=0):
        self.kind, self.eps_start, self.eps_final, self.final_step, self.n_opts = kind, eps_start, eps_final, final_step, n_opts
        self.rng = SmallRng.seed_from_u64(seed)
        self.verbose_level = verbose_level
        self.n_samples_act = self.n_samples_best_act = 0

    def eps(self) -> float:
        d = (self.eps_start - self.eps_final) / float(self.final_step)
        return max(self.eps_start - d * float(self.n_opts), self.eps_final)

    def sample(self, q, train: bool) -> np.ndarray:
        q = np.asarray(q, np.float32)
        n, A = q.shape
        best = q.argmax(1).astype(np.int64)   # numpy's argmax: the first maximum
        if not train:                         # dqn/base.rs:221-227; the ONE action goes to every row
            if self.rng.gen_f32() < F32(0.01):
                return np.full(n, self.rng.gen_range(A), np.int64)
            return best
        self.n_samples_act += 1
        if self.kind == "softmax":
            return np.array([self.rng.weighted_index(softmax_row(row)) for row in q], np.int64)
        eps = self.eps()
        r = self.rng.gen_f32()
        self.n_opts += 1
        act = np.array([self.rng.next_u64() % A for _ in range(n)], np.int64) if r < F32(eps) else best
        if self.verbose_level >= 2 and np.array_equal(act, best):
            self.n_samples_best_act += 1
        return act


if __name__ == "__main__":
    import json
    print(json.dumps({"small_rng": small_rng_kat()}, indent=1))
