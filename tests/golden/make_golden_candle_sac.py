"""Writes tests/golden/candle_sac_*.npz: initial parameters, per-step batches and N(0,1) draws, and per-step records, gradients,
probes and parameters of the float32 autograd restatement of border-candle-agent's Sac::opt_ (tests/candle_sac_restatement.py), in
train mode, and per step the float32-versus-float64 figures of the same restatement (fig_*: R.f32_f64_figures), which the GPU
test's bars refer to.  Precondition, asserted here: on every row max |a / scale| < 0.999 for a and next_a - beyond that the atanh round trip
of logp is ill-conditioned in float32 and belongs to tests/test_gpu_candle_sac_edges.py, not to a relative bar.
Run: python tests/golden/make_golden_candle_sac.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import candle_sac_restatement as R  # noqa: E402

BATCH_KEYS = ("obs", "act", "next_obs", "reward", "is_terminated", "is_truncated")
ADAMW = dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)
PROBE_KEYS = ("a", "logp", "q_min", "dq_da", "next_a", "next_logp", "tgt")
Z_SCALE = 0.4   # the draws' spread (R.CandleSacSpec.draws): keeps the Tanh limit off saturation

# name -> (spec, batch size, steps, seed)
CASES = {
    "mlp2_tanh_auto_smooth_l1": (R.CandleSacSpec(7, 3, (24, 16), (24, 24), actor_kind="Mlp2", action_limit="Tanh", action_scale=2.0,
                                                 ent_coef=("Auto", -3.0, 1e-3), critic_loss="SmoothL1"), 8, 3, 1),
    "mlp2_clamp_fix_mse_adamw": (R.CandleSacSpec(6, 2, (16, 24), (24,), actor_kind="Mlp2", ent_coef=("Fix", 0.2), lr_actor=1e-3, lr_critic=1e-3,
                                                 adamw={"actor": ADAMW, "critic": ADAMW}), 8, 3, 2),
    "mlp3_tanh_auto_three_critics": (R.CandleSacSpec(5, 4, (24,), (16, 16), actor_kind="Mlp3", n_critics=3, action_limit="Tanh",
                                                     ent_coef=("Auto", -4.0, 1e-2)), 8, 3, 3),
    # two IDENTICAL critics (every row a tie of the minimum): candle's reduce-min backward gives the action gradient to both
    "mlp2_clamp_identical_critics": (R.CandleSacSpec(6, 2, (16, 16), (24,), actor_kind="Mlp2", ent_coef=("Fix", 0.5)), 8, 3, 4),
}
IDENTICAL_CRITICS = ("mlp2_clamp_identical_critics",)


def case(name):
    return CASES[name]


def initial(name):
    spec, _, _, seed = CASES[name]
    actor, critics, tgts = spec.init_params(seed)
    if name in IDENTICAL_CRITICS:
        critics = [critics[0].copy() for _ in critics]
        tgts = [c.copy() for c in critics]
    return actor, critics, tgts


def inputs(name, s):
    """(batch, z_pi, z_next) of step s"""
    spec, bsz, _, seed = CASES[name]
    return (R.make_batch(spec, bsz, 1000 * seed + s),) + tuple(spec.draws(bsz, 1000 * seed + 500 + s, Z_SCALE))


def make(name):
    spec, bsz, steps, seed = CASES[name]
    actor, critics, tgts = initial(name)
    ref = R.CandleSacRestatement(spec, actor, critics, tgts)
    ref64 = R.CandleSacRestatement(spec, actor, critics, tgts, dtype=torch.float64)
    out = {"actor0": actor}
    for i, c in enumerate(critics):
        out[f"critic{i}_0"] = c
    for s in range(steps):
        batch, z_pi, z_next = inputs(name, s)
        for k, v in zip(BATCH_KEYS, batch):
            out[f"s{s}_{k}"] = v
        out[f"s{s}_z_pi"], out[f"s{s}_z_next"] = z_pi, z_next
        rec = ref.update(*batch, z_pi, z_next)
        ref64.update(*batch, z_pi, z_next)
        for k, v in R.f32_f64_figures(ref, ref64).items():
            out[f"s{s}_fig_{k}"] = np.float64(v)
        pr = ref.probes
        if spec.action_limit == "Tanh":
            for k in ("a", "next_a"):
                assert np.abs(pr[k] / spec.action_scale).max() < 0.999, (name, s, k, np.abs(pr[k] / spec.action_scale).max())
        for k, v in rec.items():
            out[f"s{s}_{k}"] = np.float32(v)
        for k in PROBE_KEYS:
            out[f"s{s}_{k}"] = pr[k]
        out[f"s{s}_actor_grad"], out[f"s{s}_actor"], out[f"s{s}_log_alpha"] = pr["actor_grad"], ref.params("actor"), ref.params("log_alpha")
        for i in range(spec.n_critics):
            out[f"s{s}_critic{i}_grad"] = pr["critic_grads"][i]
            out[f"s{s}_critic{i}"] = ref.params(f"critic_{i}")
            out[f"s{s}_critic_tgt{i}"] = ref.params(f"critic_tgt_{i}")
    np.savez_compressed(os.path.join(HERE, f"candle_sac_{name}.npz"), **out)


if __name__ == "__main__":
    for n in CASES:
        make(n)
        print(n, os.path.getsize(os.path.join(HERE, f"candle_sac_{n}.npz")))
