"""Writes tests/golden/candle_dqn_*.npz: initial parameters, per-step batches, and per-step records, probes, gradients and parameters of
the float32 autograd restatement of border-candle-agent's Dqn (tests/candle_dqn_restatement.py), and per step the
float32-versus-float64 figures of the same restatement (fig_*: R.f32_f64_figures), which the GPU test's bars refer to.
Precondition, asserted here for the double_dqn case: on every row the two leading online Q(next_obs) values differ by more than 1e-4
of the largest |Q|, so no row's argmax hangs on float32 round-off.
Run: python tests/golden/make_golden_candle_dqn.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import candle_dqn_restatement as R  # noqa: E402

BATCH_KEYS = ("obs", "act", "next_obs", "reward", "is_terminated", "is_truncated")
ADAMW = dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)
PROBE_KEYS = ("pred", "q_next", "y", "tgt", "dpred")

# name -> (spec, batch size, steps, seed)
CASES = {
    "mse_adamw": (R.CandleDqnSpec(4, 2, (24, 16), adamw=ADAMW), 8, 3, 1),
    "smooth_l1_adam_double": (R.CandleDqnSpec(5, 3, (16, 24), adamw=None, double_dqn=True, critic_loss="SmoothL1", lr=3e-4), 8, 3, 2),
    "soft_update_interval2_tau05": (R.CandleDqnSpec(3, 4, (16,), adamw=ADAMW, soft_update_interval=2, tau=0.5), 6, 3, 3),
    "three_hidden_relu_out": (R.CandleDqnSpec(6, 5, (16, 24, 16), relu_out=True, adamw=ADAMW), 8, 2, 4),
}


def case(name):
    return CASES[name]


def initial(name):
    spec, _, _, seed = CASES[name]
    return spec.init_params(seed)


def inputs(name, s):
    spec, bsz, _, seed = CASES[name]
    return R.make_batch(spec, bsz, 1000 * seed + s)


def make(name):
    spec, bsz, steps, seed = CASES[name]
    q0, t0 = initial(name)
    ref = R.CandleDqnRestatement(spec, q0, t0)
    ref64 = R.CandleDqnRestatement(spec, q0, t0, dtype=torch.float64)
    out = {"qnet0": q0, "qnet_tgt0": t0}
    for s in range(steps):
        batch = inputs(name, s)
        for k, v in zip(BATCH_KEYS, batch):
            out[f"s{s}_{k}"] = v
        if spec.double_dqn:
            assert R.double_dqn_gap(ref, batch[2]) > 1e-4, (name, s, R.double_dqn_gap(ref, batch[2]))
        rec = ref.update(*batch)
        ref64.update(*batch)
        for k, v in R.f32_f64_figures(ref, ref64).items():
            out[f"s{s}_fig_{k}"] = np.float64(v)
        for k, v in rec.items():
            out[f"s{s}_{k}"] = np.float32(v)
        for k in PROBE_KEYS:
            out[f"s{s}_{k}"] = ref.probes[k]
        out[f"s{s}_grad"], out[f"s{s}_qnet"], out[f"s{s}_qnet_tgt"] = ref.probes["grad"], ref.params("qnet"), ref.params("qnet_tgt")
    np.savez_compressed(os.path.join(HERE, f"candle_dqn_{name}.npz"), **out)


if __name__ == "__main__":
    for n in CASES:
        make(n)
        print(n, os.path.getsize(os.path.join(HERE, f"candle_dqn_{n}.npz")))
