"""Writes tests/golden/awac_*.npz: initial parameters, per-step batches and N(0,1) draws, and per-step records, gradients and
parameters of the float32 autograd restatement of border-candle-agent's Awac::opt_ (tests/awac_restatement.py), in train mode.
Run: python tests/golden/make_golden_awac.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import awac_restatement as R  # noqa: E402

BATCH_KEYS = ("obs", "act", "next_obs", "reward", "is_terminated", "is_truncated")
ADAMW = dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)

# name -> (spec, batch size, steps, seed)
CASES = {
    "clamp_mse": (R.AwacSpec(11, 3, (32, 32), (32, 32)), 64, 3, 1),
    "tanh_smooth_l1": (R.AwacSpec(9, 4, (24,), (24, 24), critic_loss="SmoothL1", action_limit="Tanh", action_scale=2.0), 48, 3, 2),
    "adv_softmax": (R.AwacSpec(13, 2, (32, 16), (32,), adv_softmax=True, inv_lambda=3.0), 40, 3, 3),
    "three_critics_adamw": (R.AwacSpec(10, 5, (32, 32), (32, 32), n_critics=3, lr_actor=1e-3, lr_critic=1e-3,
                                       adamw={"actor": ADAMW, "critic": ADAMW}), 56, 3, 4),
}


def case(name):
    return CASES[name]


def make(name):
    spec, bsz, steps, seed = CASES[name]
    actor, critics, tgts = spec.init_params(seed)
    ref = R.AwacRestatement(spec, actor, critics, tgts)
    out = {"actor0": actor}
    for i, c in enumerate(critics):
        out[f"critic{i}_0"] = c
    for s in range(steps):
        batch = R.make_batch(spec, bsz, 1000 * seed + s)
        z_pi, z_next = spec.draws(bsz, 1000 * seed + 500 + s)
        for k, v in zip(BATCH_KEYS, batch):
            out[f"s{s}_{k}"] = v
        out[f"s{s}_z_pi"], out[f"s{s}_z_next"] = z_pi, z_next
        rec = ref.update(*batch, z_pi, z_next)
        for k, v in rec.items():
            out[f"s{s}_{k}"] = np.float32(v)
        pr = ref.probes
        out[f"s{s}_actor_grad"], out[f"s{s}_actor"] = pr["actor_grad"], ref.params("actor")
        for i in range(spec.n_critics):
            out[f"s{s}_critic{i}_grad"] = pr["critic_grads"][i]
            out[f"s{s}_critic{i}"] = ref.params(f"critic_{i}")
            out[f"s{s}_critic_tgt{i}"] = ref.params(f"critic_tgt_{i}")
    np.savez_compressed(os.path.join(HERE, f"awac_{name}.npz"), **out)


if __name__ == "__main__":
    for n in CASES:
        make(n)
        print(n, os.path.getsize(os.path.join(HERE, f"awac_{n}.npz")))
