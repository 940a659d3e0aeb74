"""Writes the goldens of the candle DQN's AtariCnn form: tests/golden/candle_dqn_cnn_<case>.npz, one per committed case of
tests/candle_dqn_cnn_restatement.py (CASES).  A golden holds the case's seed and shapes and RESULTS of the float32 restatement only -
loss and probes of every update, the norm and a fixed sample of entries of every variable's gradient (every update), parameters and
target parameters (at the end) - never the 1.7 M parameters: parameters and batches are regenerated from the seed (case_inputs).

  python tests/golden/make_golden_candle_dqn_cnn.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import candle_dqn_cnn_restatement as R  # noqa: E402

N_SAMPLE = 24


def sample_index(name: str, n: int) -> np.ndarray:
    """the fixed sample of entries of a variable with n elements"""
    rng = np.random.default_rng(sum(name.encode()) * 7919 + n)
    return np.sort(rng.choice(n, min(N_SAMPLE, n), replace=False)).astype(np.int64)


def golden_of(c: R.Case) -> dict:
    r, steps = R.run_case(c)
    q = R.quantities(c, r, steps)
    sl = R.var_slices(c.spec.n_stack, c.spec.n_actions)
    out = dict(seed=np.int64(c.seed), batch=np.int64(c.batch), n_stack=np.int64(c.spec.n_stack), n_actions=np.int64(c.spec.n_actions),
               n_updates=np.int64(c.n_updates))
    for k, s in enumerate(steps):
        out[f"loss/{k}"] = q[f"loss/{k}"].astype(np.float32)
        out[f"y/{k}"] = s["y"].astype(np.int64)
        for key in R.PROBE_KEYS:
            out[f"{key}/{k}"] = q[f"{key}/{k}"].astype(np.float32)
        for name in R.VAR_NAMES:
            g = q[f"grad:{name}/{k}"]
            out[f"grad_norm:{name}/{k}"] = np.float64(np.sqrt((g.astype(np.float64) ** 2).sum()))
            out[f"grad_sample:{name}/{k}"] = g[sample_index(name, g.size)].astype(np.float32)
    for which in ("qnet", "qnet_tgt"):
        for name in R.VAR_NAMES:
            v = q[which][sl[name]]
            out[f"{which}_sample:{name}"] = v[sample_index(name, v.size)].astype(np.float32)
    return out


def path_of(c: R.Case) -> str:
    return os.path.join(HERE, f"candle_dqn_cnn_{c.name}.npz")


if __name__ == "__main__":
    for c in R.CASES:
        np.savez(path_of(c), **golden_of(c))
        print(path_of(c), os.path.getsize(path_of(c)))
