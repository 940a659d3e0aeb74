"""Writes tests/golden/bc_*.npz: initial parameters, per-step batches, and per-step losses, predictions, gradients and parameters of
the float32 autograd restatement of border-candle-agent's Bc::opt_ (tests/bc_restatement.py).
Run: python tests/golden/make_golden_bc.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bc_restatement as R  # noqa: E402

ADAMW = dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)

# name -> (spec, batch size, steps, seed)
CASES = {
    "tanh_adamw": (R.BcSpec(45, 24, (48, 48), "Tanh", lr=1e-3, adamw=ADAMW), 64, 3, 1),          # bc_pen's architecture, scaled down
    "none_adam": (R.BcSpec(11, 3, (32, 32), "None", lr=3e-4), 48, 3, 2),
    "sigmoid_one_hidden": (R.BcSpec(9, 4, (40,), "Sigmoid", lr=1e-3), 40, 3, 3),
    "relu_ragged_three_hidden": (R.BcSpec(13, 7, (48, 33, 20), "ReLU", lr=1e-3, adamw=ADAMW), 37, 3, 4),
}


def case(name):
    return CASES[name]


def make(name):
    spec, bsz, steps, seed = CASES[name]
    p0 = spec.init_params(seed)
    ref = R.BcRestatement(spec, p0)
    out = {"policy0": p0}
    for s in range(steps):
        obs, act = R.make_batch(spec, bsz, 1000 * seed + s)
        out[f"s{s}_obs"], out[f"s{s}_act"] = obs, act
        rec = ref.update(obs, act)
        out[f"s{s}_loss"] = np.float32(rec["loss"])
        out[f"s{s}_pred"], out[f"s{s}_dz"] = ref.probes["pred"], ref.probes["dz"]
        out[f"s{s}_grad"], out[f"s{s}_policy"] = ref.probes["grad"], ref.params()
    np.savez_compressed(os.path.join(HERE, f"bc_{name}.npz"), **out)


if __name__ == "__main__":
    for n in CASES:
        make(n)
        print(n, os.path.getsize(os.path.join(HERE, f"bc_{n}.npz")))
