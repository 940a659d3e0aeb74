"""The gather's grid of a BC and of an IQL group (csrc/group_core.hpp group_create): the plan checks the grid of replay_gather_shape's
rule against the launch limits, the launch takes replay_gather_shape's own grid, and the diagnostics override BDR_GATHER_CHUNKS can make
the two differ.  Both kinds refuse the group then, on the host, before any launch, and leave no agent behind.  The override is read once
per process, so each case runs in a fresh child process."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

# obs 4 (rows of 16 bytes: the vector path the override applies to), act 2, one hidden layer of 64, B = 33, one member
CHILD = r"""
import sys
import border_amd as B
from border_amd.iql import CandleMlpConfig, GaussianActorConfig, IqlConfig, MultiCriticConfig, ValueConfig

override = sys.argv[1] == "override"
made = []
for cls in (B.Bc, B.Iql):
    def init(self, config, _init=cls.__init__):
        _init(self, config)
        made.append(self)
    cls.__init__ = init
mlp, adam = CandleMlpConfig((64,), "None"), B.OptimizerConfig.Adam(1e-3)
bc = B.BcConfig(obs_dim=4, act_dim=2, policy_model_config=B.BcModelConfig(mlp, adam), batch_size=33, action_type="Continuous", device=0, seed=1,
                kernel_form="general")
iql = IqlConfig(obs_dim=4, act_dim=2, value_config=ValueConfig(mlp, adam), critic_config=MultiCriticConfig(2, mlp, adam, 0.005),
                actor_config=GaussianActorConfig(mlp, adam), batch_size=33, seed=1, device=0)
for kind, group, config in (("BC", B.BcGroup, bc), ("IQL", B.IqlGroup, iql)):
    del made[:]
    try:
        g = group.build([config])
    except B.BdrError as e:
        assert override, str(e)
        assert "the gather's grid (2 workgroups per row)" in str(e) and f"no {kind} group" in str(e), str(e)
        assert len(made) == 1 and made[0].handle is None, made   # the one agent built for the group is closed again
    else:
        assert not override, kind
        assert len(g) == 1 and g.kernel_launches == 0
        g.close()
    print(kind, "refused" if override else "built")
"""


@pytest.mark.parametrize("override", [True, False])
def test_both_kinds_refuse_a_group_whose_gather_grid_is_not_the_plans(override):
    env = {k: v for k, v in os.environ.items() if k != "BDR_GATHER_CHUNKS"}
    if override: env["BDR_GATHER_CHUNKS"] = "2"
    r = subprocess.run([sys.executable, "-c", CHILD, "override" if override else "plain"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    word = "refused" if override else "built"
    assert r.stdout.split() == ["BC", word, "IQL", word], r.stdout
