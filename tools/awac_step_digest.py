"""One line: the sha256 over every model's parameters, both Adam moments and the critics' targets of a standalone AWAC agent after five
update_on_batch steps at the pen shape (obs 45, act 24, critic / actor Mlp[256, 256, 256], two critics, B = 256) in train mode on the
device noise stream (no host draws: act_ and next_act come from the agent's own counter), with a fixed seed and fixed rows.  AWAC's GPU
tests are tolerance tests; this digest is how a change that must not move the standalone path is checked bit for bit: run it against
two builds of the library (BORDER_AMD_LIB=<path to libborder_amd.so> selects one) and compare the lines."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import border_amd as B  # noqa: E402
from border_amd.iql import CandleMlpConfig, GaussianActorConfig, MultiCriticConfig  # noqa: E402

OBS, ACT, UNITS, BATCH, STEPS = 45, 24, (256, 256, 256), 256, 5


def main():
    opt = lambda: B.OptimizerConfig.Adam(3e-4)
    a = B.Awac.build(B.AwacConfig(obs_dim=OBS, act_dim=ACT, critic_config=MultiCriticConfig(2, CandleMlpConfig(UNITS), opt(), 0.005),
                                  actor_config=GaussianActorConfig(CandleMlpConfig(UNITS), opt()), batch_size=BATCH, train=True, seed=11, device=0))
    assert a.is_train()
    rng = np.random.default_rng(7)
    for _ in range(STEPS):
        a.update_on_batch(rng.standard_normal((BATCH, OBS)).astype(np.float32), rng.uniform(-0.9, 0.9, (BATCH, ACT)).astype(np.float32),
                          rng.standard_normal((BATCH, OBS)).astype(np.float32), rng.standard_normal(BATCH).astype(np.float32),
                          (rng.random(BATCH) < 0.1).astype(np.int8), np.zeros(BATCH, np.int8))
    h = hashlib.sha256()
    for model in ("actor", "critic_0", "critic_1"):
        for role in ("param", "exp_avg", "exp_avg_sq"):
            h.update(a.get_params(model, role=role).tobytes())
    for model in ("critic_tgt_0", "critic_tgt_1"):
        h.update(a.get_params(model).tobytes())
    h.update(a.probe("act_", BATCH).tobytes())   # the last step's draws: the stream itself
    a.close()
    print("awac pen, train mode, %d update_on_batch steps, seed 11: sha256 %s" % (STEPS, h.hexdigest()))


if __name__ == "__main__":
    main()
