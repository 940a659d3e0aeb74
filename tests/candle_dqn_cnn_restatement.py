"""Independent restatement of border-candle-agent's Dqn with the AtariCnn Q-network (atari_cnn/base.rs:31-45): the checker of the
AtariCnn form of the HIP candle DQN agent (csrc/candle_dqn.hip, CandleDqnCnn).  Nothing under border_amd/ imports this file, and
nothing here runs candle: this file IS the statement of what the device is held to.

  AtariCnn                   obs u8 [B][n_stack * 84 * 84] -> to f32 / f64, `x / 255` PER ELEMENT, conv2d (cross-correlation, as
                             candle_nn::conv2d and torch.nn.functional.conv2d) 8x8/4, 4x4/2, 3x3/1 with ReLU after each, the (c, h, w)
                             flatten, l1 3136 -> 512, ReLU, l2 512 -> A.  Variables in checkpoint order: c1.weight [32][ns][8][8],
                             c1.bias, c2.weight [64][32][4][4], c2.bias, c3.weight [64][64][3][3], c3.bias, l1.weight [512][3136],
                             l1.bias, l2.weight [A][512], l2.bias.
  CandleDqnCnnRestatement    tests/candle_dqn_restatement.py's CandleDqnRestatement with that network: update_critic, opt_, track and
                             the optimizer rules are INHERITED, not copied.

The device scales by 1/255 where the shared conv1 kernel scales (its epilogue: one multiplication of the accumulated sum by
f32(1/255)), not per element: a rounding-level difference that the tolerance rule covers; it is not a bit contract.  Parameter
initialisation is the library's own seeded initialiser; tests set parameters.

Tolerances.  For each compared quantity the bar is 4 x the largest distance between the float32 and the float64 evaluation of this
restatement over the committed cases (CASES); the factor 4 is for the device's accumulation order.  F32_F64 holds
those largest distances as measured on the CPU with torch on one thread (single_thread: the split of the work moves the float32
results); tests/test_candle_dqn_cnn_restatement.py recomputes them and fails when they drift.
A ReLU unit within rounding of zero can be masked differently on the device and flip a gradient term, so every case is built such
that no pre-activation of the float64 evaluation of the gradient pass - Q(obs) of the online net, the only pass a gradient flows
through; a flip in the other passes moves values continuously - lies within 64 x that layer's float32-versus-float64 forward distance
of zero, and no argmax row of the passes that pick an action hangs on less than 64 x the Q distance.  A seed search alone cannot do
that: a frame stack has 12 800 + 5 184 + 3 136 + 512 units per row, and with every parameter drawn at random the smallest
|pre-activation| of a batch of 8 measured 2 000 x too small (of one row: 7 x).  So the weights come from the seed and the four ReLU
layers' biases of the online net are then placed (margin_biases): per output channel, minus the midpoint of the widest gap among the
central 40 % of the channel's sorted bias-free pre-activations over the observations of all of the case's updates - about half of a
channel's units stay open, and every unit keeps half that gap (1e-3 and more) from zero.  The cases step with lr 1e-7 (a conv1 channel's 256 weights move together under Adam: lr 1e-5 shifted its units by 1e-3) so that the
second and third update still see those margins; the seed is then searched (find_seed) for the precondition to hold at every
update.  The CPU test asserts the precondition for every committed case.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as TF

from candle_dqn_restatement import AdamState, CandleDqnRestatement, _cast, rel

def single_thread(fn):
    """Run fn with torch on ONE thread: the float32 results of conv2d and matmul depend on how the work is split (the committed
    cases' grad:c1.bias distance measured 9.3e-7 on many threads and 2.2e-6 on one), and the committed figures must regenerate on
    any machine."""
    @functools.wraps(fn)
    def wrapped(*a, **k):
        n = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            return fn(*a, **k)
        finally:
            torch.set_num_threads(n)
    return wrapped


VAR_NAMES = ("c1.weight", "c1.bias", "c2.weight", "c2.bias", "c3.weight", "c3.bias", "l1.weight", "l1.bias", "l2.weight", "l2.bias")


def var_shapes(n_stack: int, A: int):
    return [(32, n_stack, 8, 8), (32,), (64, 32, 4, 4), (64,), (64, 64, 3, 3), (64,), (512, 3136), (512,), (A, 512), (A,)]


def var_slices(n_stack: int, A: int) -> dict:
    out, o = {}, 0
    for name, s in zip(VAR_NAMES, var_shapes(n_stack, A)):
        n = int(np.prod(s))
        out[name] = slice(o, o + n)
        o += n
    return out


class AtariCnn:
    """atari_cnn/base.rs:31-45.  The three keyword flags are the mutations of tests/test_candle_dqn_cnn_restatement.py."""

    def __init__(self, n_stack: int, A: int, flat, no_div255=False, hwc_flatten=False, no_relu3=False):
        self.n_stack, self.A = n_stack, A
        self.no_div255, self.hwc_flatten, self.no_relu3 = no_div255, hwc_flatten, no_relu3
        self.params, o = [], 0
        for s in var_shapes(n_stack, A):
            n = int(np.prod(s))
            self.params.append(torch.tensor(np.asarray(flat[o:o + n], np.float32).reshape(s), requires_grad=True))
            o += n
        assert o == len(flat), (o, len(flat))

    def forward(self, x, trace: Optional[list] = None):
        """x [B][n_stack * 84 * 84]: the u8 values as floats of the parameters' dtype.  trace: receives the four pre-activations."""
        w1, b1, w2, b2, w3, b3, w4, b4, w5, b5 = self.params
        x = x.reshape(-1, self.n_stack, 84, 84)        # [B, n_stack, 1, 84, 84].squeeze(2)
        if not self.no_div255:
            x = x / 255.0                              # to_dtype(F32) / 255.0: one division per element
        z1 = TF.conv2d(x, w1, b1, stride=4)
        z2 = TF.conv2d(torch.relu(z1), w2, b2, stride=2)
        z3 = TF.conv2d(torch.relu(z2), w3, b3, stride=1)
        a3 = z3 if self.no_relu3 else torch.relu(z3)
        f = (a3.permute(0, 2, 3, 1) if self.hwc_flatten else a3).flatten(1)   # flatten_from(1) of [B, 64, 7, 7]: (c, h, w)
        z4 = f @ w4.T + b4
        if trace is not None:
            trace.extend([z1, z2, z3, z4])
        return torch.relu(z4) @ w5.T + b5


@dataclass
class CandleDqnCnnSpec:
    n_stack: int
    n_actions: int
    lr: float = 1e-3
    adamw: Optional[dict] = field(default_factory=dict)   # AdamW kwargs (beta1, beta2, eps, wd); None: candle-optimisers' Adam
    gamma: float = 0.99
    tau: float = 0.005
    soft_update_interval: int = 1
    n_updates_per_opt: int = 1
    double_dqn: bool = False
    critic_loss: str = "Mse"

    @property
    def row_bytes(self) -> int:
        return 84 * 84 * self.n_stack

    def count(self) -> int:
        return sum(int(np.prod(s)) for s in var_shapes(self.n_stack, self.n_actions))

    def init_flat(self, rng) -> np.ndarray:
        out = []
        for s in var_shapes(self.n_stack, self.n_actions):
            fan_in = int(np.prod(s[1:])) if len(s) > 1 else None
            if fan_in is not None:
                bound = 1.0 / np.sqrt(fan_in)
            out.append(rng.uniform(-bound, bound, int(np.prod(s))))   # (a bias takes its weight's bound)
        return np.concatenate(out).astype(np.float32)

    def init_params(self, seed: int):
        """(qnet, qnet_tgt) in the reference layout; the target differs from the online net, as it does after the first updates"""
        rng = np.random.default_rng(seed)
        return self.init_flat(rng), self.init_flat(rng)

    def to_config(self, B, batch_size: int, **kw):
        """the border_amd.CandleDqnConfig of this spec"""
        opt = B.OptimizerConfig.Adam(self.lr) if self.adamw is None else B.OptimizerConfig.AdamW(self.lr, **self.adamw)
        return B.CandleDqnConfig(
            q_config=B.AtariCnnConfig(n_stack=self.n_stack, out_dim=self.n_actions), model_config=B.CandleDqnModelConfig(opt_config=opt),
            soft_update_interval=self.soft_update_interval, n_updates_per_opt=self.n_updates_per_opt, batch_size=batch_size,
            discount_factor=self.gamma, tau=self.tau, double_dqn=self.double_dqn, critic_loss=self.critic_loss, **kw)


def make_batch(spec: CandleDqnCnnSpec, n: int, seed: int, p_done: float = 0.2):
    """u8 frame stacks; row 0 is terminal in every batch"""
    rng = np.random.default_rng(seed)
    obs = rng.integers(0, 256, (n, spec.row_bytes), dtype=np.uint8)
    next_obs = rng.integers(0, 256, (n, spec.row_bytes), dtype=np.uint8)
    act = rng.integers(0, spec.n_actions, n).astype(np.int64)
    reward = rng.standard_normal(n).astype(np.float32)
    term = (rng.random(n) < p_done).astype(np.int8)
    term[0] = 1
    trunc = (rng.random(n) < p_done).astype(np.int8)
    return obs, act, next_obs, reward, term, trunc


class CandleDqnCnnRestatement(CandleDqnRestatement):
    """update_critic / opt_ / update / track / params: CandleDqnRestatement's, on two AtariCnn networks"""

    def __init__(self, spec: CandleDqnCnnSpec, qnet, qnet_tgt, dtype=torch.float32, **mutation):
        s = self.spec = spec
        self.dtype = dtype
        self.qnet = _cast(AtariCnn(s.n_stack, s.n_actions, np.asarray(qnet, np.float32), **mutation), dtype)
        self.qnet_tgt = _cast(AtariCnn(s.n_stack, s.n_actions, np.asarray(qnet_tgt, np.float32), **mutation), dtype)
        self.opt = AdamState(self.qnet.params, s.lr, adamw=s.adamw is not None, **(s.adamw or {}))
        self.soft_update_counter = 0
        self.n_opts = 0

    def pre_activations(self, net: AtariCnn, obs) -> list:
        with torch.no_grad():
            tr = []
            net.forward(torch.as_tensor(np.asarray(obs, np.float32)).to(self.dtype), tr)
            return [z.numpy() for z in tr]

    def param_stats(self) -> dict:
        out = {}
        for name, p in zip(VAR_NAMES, self.qnet.params):
            v = p.detach().numpy().astype(np.float64)
            out[f"{name}_mean"], out[f"{name}_std"] = float(v.mean()), float(v.std())
        return out


# ------------------------------------------------------------------------------------------------ committed cases
@dataclass
class Case:
    name: str
    spec: CandleDqnCnnSpec
    batch: int
    seed: int            # chosen by find_seed: parameters from `seed`, update k's batch from seed + 1 + k
    n_updates: int = 2
    tie: bool = False    # an exact tie of the two largest target-net values in every row (l2 rows 0 and 1 of qnet_tgt made equal)


def margin_biases(spec: CandleDqnCnnSpec, flat: np.ndarray, obs_all: np.ndarray) -> np.ndarray:
    """the biases of c1, c2, c3, l1 of `flat` placed as the module docstring says, layer by layer in float64"""
    flat = flat.copy()
    sl = var_slices(spec.n_stack, spec.n_actions)
    x = torch.as_tensor(np.asarray(obs_all, np.float32)).to(torch.float64)
    for k, name in enumerate(("c1.bias", "c2.bias", "c3.bias", "l1.bias")):
        flat[sl[name]] = 0
        net = _cast(AtariCnn(spec.n_stack, spec.n_actions, flat), torch.float64)
        with torch.no_grad():
            tr = []
            net.forward(x, tr)
        z = tr[k].numpy()
        z = np.sort(np.moveaxis(z, 1, 0).reshape(z.shape[1], -1), axis=1)      # [channel][sorted values]
        n = z.shape[1]
        lo, hi = int(0.3 * n), max(int(0.7 * n), int(0.3 * n) + 2)
        gaps = np.diff(z[:, lo:hi], axis=1)
        j = gaps.argmax(1) + lo
        rows = np.arange(z.shape[0])
        flat[sl[name]] = (-(z[rows, j] + z[rows, j + 1]) / 2).astype(np.float32)
    return flat


@single_thread
def case_inputs(c: Case):
    qnet, qnet_tgt = c.spec.init_params(c.seed)
    qnet = margin_biases(c.spec, qnet, np.concatenate([make_batch(c.spec, c.batch, c.seed + 1 + k)[0] for k in range(c.n_updates)]))
    if c.tie:   # rows 0 and 1 of the target's l2 are the same and win every row: the first maximum is index 0
        sl = var_slices(c.spec.n_stack, c.spec.n_actions)
        w = qnet_tgt[sl["l2.weight"]].reshape(c.spec.n_actions, 512)
        b = qnet_tgt[sl["l2.bias"]]
        w[1] = w[0]
        b[0] = b[1] = np.float32(4.0)
    batches = [make_batch(c.spec, c.batch, c.seed + 1 + k) for k in range(c.n_updates)]
    return qnet, qnet_tgt, batches


CASES = (
    Case("b8_ns4_a6_mse_adamw", CandleDqnCnnSpec(4, 6, lr=1e-7, adamw=dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)), 8, seed=1000),
    Case("b3_ns1_a18_smoothl1_ddqn_adam", CandleDqnCnnSpec(1, 18, lr=1e-7, adamw=None, double_dqn=True, critic_loss="SmoothL1"), 3, seed=2000, n_updates=3),
    Case("b1_ns4_a2_mse_tie_adamw", CandleDqnCnnSpec(4, 2, lr=1e-7, adamw=dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01), tau=0.05, soft_update_interval=3), 1, seed=3001, tie=True),
)

PROBE_KEYS = ("pred", "q_next", "tgt", "dpred")


@single_thread
def run_case(c: Case, dtype=torch.float32, **mutation):
    """the case's updates on one restatement: (restatement, per-update list of {loss, probes..., grad})"""
    qnet, qnet_tgt, batches = case_inputs(c)
    r = CandleDqnCnnRestatement(c.spec, qnet, qnet_tgt, dtype, **mutation)
    steps = []
    for b in batches:
        rec = r.update(*b)
        steps.append(dict(loss=rec["loss"], **{k: np.array(v) for k, v in r.probes.items()}))
    return r, steps


def quantities(c: Case, r: CandleDqnCnnRestatement, steps) -> dict:
    """every compared quantity of a finished case, by name: probes and loss of every update, the ten gradients of every update, the
    parameters and target parameters at the end"""
    sl = var_slices(c.spec.n_stack, c.spec.n_actions)
    out = {}
    for k, s in enumerate(steps):
        out[f"loss/{k}"] = np.asarray([s["loss"]])
        for key in PROBE_KEYS:
            out[f"{key}/{k}"] = s[key]
        for name in VAR_NAMES:
            out[f"grad:{name}/{k}"] = s["grad"][sl[name]]
    out["qnet"], out["qnet_tgt"] = r.params("qnet"), r.params("qnet_tgt")
    return out


def kind_of(qname: str) -> str:
    return qname.split("/")[0]


def distance(kind: str, a, b) -> float:
    """max-absolute for the parameters (`qnet`), max-relative (to the largest reference magnitude) for everything else - the
    measures of tests/candle_dqn_restatement.py's f32_f64_figures"""
    if kind == "qnet":
        return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
    return rel(a, b)


def f32_f64_distances(cases=CASES) -> dict:
    """the largest float32-versus-float64 distance of every quantity kind over the cases"""
    out = {}
    for c in cases:
        q32, q64 = quantities(c, *run_case(c, torch.float32)), quantities(c, *run_case(c, torch.float64))
        for name in q32:
            k = kind_of(name)
            out[k] = max(out.get(k, 0.0), distance(k, q32[name], q64[name]))
    return out


# The largest float32-versus-float64 distances over CASES, as `python tests/candle_dqn_cnn_restatement.py` prints them.  BAR[k] is
# what the device is held to against the float32 restatement.
F32_F64 = {
    "loss": 1.003e-07, "pred": 4.277e-07, "q_next": 2.012e-07, "tgt": 4.796e-08, "dpred": 5.145e-08,
    "grad:c1.weight": 1.952e-06, "grad:c1.bias": 2.231e-06, "grad:c2.weight": 1.007e-06, "grad:c2.bias": 5.776e-07,
    "grad:c3.weight": 9.002e-07, "grad:c3.bias": 6.136e-07, "grad:l1.weight": 1.335e-06, "grad:l1.bias": 9.774e-08,
    "grad:l2.weight": 2.383e-06, "grad:l2.bias": 5.812e-08,
    "qnet": 8.732e-08,       # absolute.  (The cases step by lr = 1e-7: this bar does not resolve one step; the optimizer rule is held bit for bit by
                             # tests/test_gpu_candle_dqn_cnn.py's element-by-element test instead.)
    "qnet_tgt": 1.554e-07,
}
BAR = {k: 4.0 * v for k, v in F32_F64.items()}
DRIFT = 2.0   # the CPU test fails when a recomputed distance leaves [F32_F64 / DRIFT, F32_F64 * DRIFT] (another BLAS / thread count moves the last bits)


@single_thread
def precondition(c: Case) -> dict:
    """per layer: the smallest |pre-activation| of the float64 gradient pass over 64 x the float32-versus-float64 forward distance
    of that layer (> 1 required), for every update of the case at the parameters that update sees; `argmax`: the same ratio for the
    top-two gap of the rows that pick an action (the tie case: the gap below the tied pair, and the pair must be exactly equal)."""
    qnet, qnet_tgt, batches = case_inputs(c)
    r32, r64 = CandleDqnCnnRestatement(c.spec, qnet, qnet_tgt, torch.float32), CandleDqnCnnRestatement(c.spec, qnet, qnet_tgt, torch.float64)
    out = {}
    for b in batches:
        z32, z64 = r32.pre_activations(r32.qnet, b[0]), r64.pre_activations(r64.qnet, b[0])
        for name, a, e in zip(("c1", "c2", "c3", "l1"), z32, z64):
            d = float(np.abs(a - e).max())
            out[name] = min(out.get(name, np.inf), float(np.abs(e).min()) / (64.0 * d))
        pick32, pick64 = (r32.qnet, r64.qnet) if c.spec.double_dqn else (r32.qnet_tgt, r64.qnet_tgt)
        with torch.no_grad():
            f = lambda r, net: net.forward(torch.as_tensor(np.asarray(b[2], np.float32)).to(r.dtype)).numpy().astype(np.float64)
            q32, q64 = f(r32, pick32), f(r64, pick64)
        d = float(np.abs(q32 - q64).max())
        top = np.sort(q64, axis=1)
        if c.tie:
            assert np.array_equal(q32[:, 0], q32[:, 1]) and (q32.argmax(1) == 0).all(), "the tie case must tie actions 0 and 1 at the top"
            gap = (top[:, -1] - top[:, -3]).min() if q64.shape[1] > 2 else np.inf
        else:
            gap = (top[:, -1] - top[:, -2]).min()
        out["argmax"] = min(out.get("argmax", np.inf), float(gap) / (64.0 * d))
        r32.update(*b); r64.update(*b)
    return out


def find_seed(c: Case, start: int, tries: int = 50) -> int:
    for seed in range(start, start + tries):
        cand = Case(c.name, c.spec, c.batch, seed, c.n_updates, c.tie)
        if min(precondition(cand).values()) > 1.0:
            return seed
    raise RuntimeError(f"no seed in [{start}, {start + tries}) meets the precondition of {c.name}")


if __name__ == "__main__":
    import json
    import sys
    if "--seeds" in sys.argv:
        for c in CASES:
            print(c.name, find_seed(c, c.seed - c.seed % 1000), flush=True)
    else:
        print(json.dumps({"F32_F64": f32_f64_distances(), "precondition": {c.name: precondition(c) for c in CASES}}, indent=1))
