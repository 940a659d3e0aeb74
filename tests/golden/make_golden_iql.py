"""Writes tests/golden/iql_*.npz: initial parameters, per-step batches, and per-step losses, gradients and parameters of the float32
autograd restatement of border-candle-agent's Iql::opt_ (tests/iql_restatement.py).  Run: python tests/golden/make_golden_iql.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import iql_restatement as R  # noqa: E402

BATCH_KEYS = ("obs", "act", "next_obs", "reward", "is_terminated", "is_truncated")
ADAMW = dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)

# name -> (spec, batch size, steps, seed)
CASES = {
    "clamp_mse": (R.IqlSpec(11, 3, (32, 32), (32, 32), (32, 32)), 64, 3, 1),
    "tanh_smooth_l1": (R.IqlSpec(9, 4, (24, 24), (24,), (24, 24), critic_loss="SmoothL1", action_limit="Tanh", action_scale=2.0), 48, 3, 2),
    "adv_softmax": (R.IqlSpec(13, 2, (32,), (32, 16), (32,), adv_softmax=True, inv_lambda=3.0), 40, 3, 3),
    "three_critics_adamw": (R.IqlSpec(10, 5, (32, 32), (32, 32), (32, 32), n_critics=3, lr_value=1e-3, lr_actor=1e-3, lr_critic=1e-3,
                                      adamw={"value": ADAMW, "actor": ADAMW, "critic": ADAMW}), 56, 3, 4),
}


def case(name):
    return CASES[name]


def make(name):
    spec, bsz, steps, seed = CASES[name]
    actor, critics, tgts, value = spec.init_params(seed)
    ref = R.IqlRestatement(spec, actor, critics, tgts, value)
    out = {"actor0": actor, "value0": value}
    for i, c in enumerate(critics):
        out[f"critic{i}_0"] = c
    for s in range(steps):
        batch = R.make_batch(spec, bsz, 1000 * seed + s)
        for k, v in zip(BATCH_KEYS, batch):
            out[f"s{s}_{k}"] = v
        rec = ref.update(*batch)
        for k, v in rec.items():
            out[f"s{s}_{k}"] = np.float32(v)
        pr = ref.probes
        out[f"s{s}_actor_grad"], out[f"s{s}_value_grad"] = pr["actor_grad"], pr["value_grad"]
        out[f"s{s}_actor"], out[f"s{s}_value"] = ref.params("actor"), ref.params("value")
        for i in range(spec.n_critics):
            out[f"s{s}_critic{i}_grad"] = pr["critic_grads"][i]
            out[f"s{s}_critic{i}"] = ref.params(f"critic_{i}")
            out[f"s{s}_critic_tgt{i}"] = ref.params(f"critic_tgt_{i}")
    np.savez_compressed(os.path.join(HERE, f"iql_{name}.npz"), **out)


if __name__ == "__main__":
    for n in CASES:
        make(n)
        print(n, os.path.getsize(os.path.join(HERE, f"iql_{n}.npz")))
