"""One line: the sha256 over every model's parameters, both Adam moments, the critics' targets and log_alpha of a standalone candle SAC
agent after five update_on_batch steps at the pen shape (obs 45, act 24, critic Mlp[256, 256] x 2, an Mlp2 actor [256, 256], Tanh limit,
Auto entropy coefficient, B = 256) in train mode on the device noise stream (no host draws: a and next_a come from the agent's own
counter), with a fixed seed and fixed rows, and over the last step's a.  This digest is how a change that must not move the standalone
path is checked bit for bit: run it against two builds of the library (BORDER_AMD_LIB=<path to libborder_amd.so> selects one; a
library without this commit's symbols needs its own copy of the package on the path) and compare the lines."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import border_amd as B  # noqa: E402
from border_amd.iql import ActionLimit, CandleMlpConfig, GaussianActorConfig, MultiCriticConfig  # noqa: E402

OBS, ACT, UNITS, BATCH, STEPS = 45, 24, (256, 256), 256, 5


def main():
    opt = lambda: B.OptimizerConfig.Adam(3e-4)
    a = B.CandleSac.build(B.CandleSacConfig(obs_dim=OBS, act_dim=ACT, critic_config=MultiCriticConfig(2, CandleMlpConfig(UNITS), opt(), 0.005),
                                            actor_config=GaussianActorConfig(CandleMlpConfig(UNITS), opt(), action_limit=ActionLimit.Tanh(1.0), kind="Mlp2"),
                                            ent_coef_mode=B.EntCoefMode.Auto(-float(ACT), 3e-4), batch_size=BATCH, train=True, seed=11, device=0))
    assert a.is_train()
    rng = np.random.default_rng(7)
    for _ in range(STEPS):
        a.update_on_batch(rng.standard_normal((BATCH, OBS)).astype(np.float32), rng.uniform(-0.9, 0.9, (BATCH, ACT)).astype(np.float32),
                          rng.standard_normal((BATCH, OBS)).astype(np.float32), rng.standard_normal(BATCH).astype(np.float32),
                          (rng.random(BATCH) < 0.1).astype(np.int8), np.zeros(BATCH, np.int8))
    h = hashlib.sha256()
    for model in ("actor", "critic_0", "critic_1", "log_alpha"):
        for role in ("param", "exp_avg", "exp_avg_sq"):
            h.update(a.get_params(model, role=role).tobytes())
    for model in ("critic_tgt_0", "critic_tgt_1"):
        h.update(a.get_params(model).tobytes())
    h.update(a.probe("a", BATCH).tobytes())   # the last step's draws: the stream itself
    a.close()
    print("candle sac pen, Mlp2, train mode, %d update_on_batch steps, seed 11: sha256 %s" % (STEPS, h.hexdigest()))


if __name__ == "__main__":
    main()
