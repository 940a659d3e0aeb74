"""What tests/test_gpu_group_copy.py and tests/test_gpu_hyper.py share: for each dense agent kind (BC, IQL, AWAC, the candle SAC) a
config built from a dict of its settable hyperparameters (the names of border_amd._lib.HYPER_IDS), the shapes, rings over views of one
dataset, and a member's whole training state through the parameter views.

Shapes, the smallest at which a kernel can still go wrong (those of the group tests) and one whose segments span several workgroups:
  bc          partial_block (17, 6, (64, 48), B 7) in the general and the MFMA head form; head_nt2 (21, 40, (64,), B 33); wide (256, 256)
  iql         partial_block; unequal (value (64,), critic (64, 64, 64), actor (128,): arenas of unequal length); wide (256, 256)
  awac        partial_block; unequal (critic (64, 64, 64), actor (128,)); wide (256, 256)
  candle_sac  partial_block (Mlp2); unequal (Mlp3, critic (64, 64, 64), actor (128,)); wide (256, 256) (Mlp2)
Every optimizer is AdamW, so that the betas, eps and the weight decay are read."""
import numpy as np

ROLES = ("param", "grad", "exp_avg", "exp_avg_sq")
N_ROWS = 100

# kind -> name -> (obs, act, {network: units}, batch, extra)
SHAPES = {
    "bc": {
        "partial_block": (17, 6, {"policy": (64, 48)}, 7, "general"),
        "partial_block_mfma": (17, 6, {"policy": (64, 48)}, 7, "fused_mfma"),
        "head_nt2": (21, 40, {"policy": (64,)}, 33, "fused_mfma"),
        "wide": (45, 24, {"policy": (256, 256)}, 40, "general"),
    },
    "iql": {
        "partial_block": (17, 6, {"value": (64, 48), "critic": (64, 48), "actor": (64, 48)}, 7, None),
        "unequal": (21, 40, {"value": (64,), "critic": (64, 64, 64), "actor": (128,)}, 20, None),
        "wide": (45, 24, {"value": (256, 256), "critic": (256, 256), "actor": (256, 256)}, 40, None),
    },
    "awac": {
        "partial_block": (17, 6, {"critic": (64, 48), "actor": (64, 48)}, 7, None),
        "unequal": (21, 40, {"critic": (64, 64, 64), "actor": (128,)}, 20, None),
        "wide": (45, 24, {"critic": (256, 256), "actor": (256, 256)}, 40, None),
    },
    "candle_sac": {
        "partial_block": (17, 6, {"critic": (64, 48), "actor": (64, 48)}, 7, "Mlp2"),
        "unequal": (21, 40, {"critic": (64, 64, 64), "actor": (128,)}, 20, "Mlp3"),
        "wide": (45, 24, {"critic": (256, 256), "actor": (256, 256)}, 41, "Mlp2"),
    },
}
CASES = [(k, n) for k, s in SHAPES.items() for n in s]
NETS = {"bc": ("",), "iql": ("value", "critic", "actor"), "awac": ("critic", "actor"), "candle_sac": ("critic", "actor")}
SCALARS = {"bc": (), "iql": ("gamma", "critic_tau", "tau_iql", "inv_lambda", "exp_adv_max"), "awac": ("gamma", "critic_tau", "inv_lambda", "exp_adv_max"),
           "candle_sac": ("gamma", "critic_tau", "ent_coef_lr", "target_entropy")}
GROUPS = {"bc": "BcGroup", "iql": "IqlGroup", "awac": "AwacGroup", "candle_sac": "CandleSacGroup"}
AGENTS = {"bc": "Bc", "iql": "Iql", "awac": "Awac", "candle_sac": "CandleSac"}
HAS_MODE = {"bc": False, "iql": True, "awac": True, "candle_sac": True}


def opt_names(net):
    """the five hyperparameter names of a network's optimizer: its learning rate, beta1, beta2, eps, weight_decay"""
    if net == "":
        return ["lr", "beta1", "beta2", "eps", "weight_decay"]
    return ["lr_" + net] + [f"{net}_{s}" for s in ("beta1", "beta2", "eps", "weight_decay")]


def hyper_names(kind, auto=True):
    """every settable hyperparameter of the kind (a candle SAC agent with a fixed entropy coefficient has neither ent_coef_lr nor target_entropy)"""
    names = [n for net in NETS[kind] for n in opt_names(net)] + list(SCALARS[kind])
    return [n for n in names if auto or n not in ("ent_coef_lr", "target_entropy")]


def hypers(kind, i, act_dim=6, auto=True):
    """member i's hyperparameters: every one differs from member 0's"""
    h = {}
    for k, net in enumerate(NETS[kind]):
        lr, b1, b2, eps, wd = opt_names(net)
        h.update({lr: (1e-3, 2e-3, 5e-4)[k] * (1 + 0.5 * i), b1: 0.9 - 0.02 * i - 0.01 * k, b2: 0.999 - 0.004 * i - 0.001 * k, eps: 1e-8 * (1 + i + k),
                  wd: 0.02 * (1 + i) + 0.005 * k})
    s = {"gamma": 0.99 - 0.02 * i, "critic_tau": 0.005 * (1 + i), "tau_iql": 0.7 + 0.04 * i, "inv_lambda": 3.0 / (1 + i), "exp_adv_max": 100.0 / (1 + 3 * i),
         "ent_coef_lr": 3e-3 * (1 + i), "target_entropy": -0.5 * act_dim * (1 + 0.1 * i)}
    h.update({n: s[n] for n in SCALARS[kind]})
    return {n: h[n] for n in hyper_names(kind, auto)}


def other_value(name, v):
    """another valid value of hyperparameter `name`"""
    if name.endswith("beta1") or name.endswith("beta2") or name in ("gamma", "tau_iql"):
        return v - 0.05
    if name == "target_entropy":
        return v - 1.0
    return v * 1.7


def config(B, kind, shape, h, seed, train=True, alpha=0.3):
    """the kind's config from the hyperparameters `h` (no ent_coef_lr in it: a candle SAC agent with Fix(alpha))"""
    from border_amd.iql import ActionLimit, CandleMlpConfig, GaussianActorConfig, IqlConfig, MultiCriticConfig, ValueConfig
    od, ad, units, bsz, extra = shape

    def opt(net):
        lr, b1, b2, eps, wd = (h[n] for n in opt_names(net))
        return B.OptimizerConfig.AdamW(lr, b1, b2, wd, eps)
    if kind == "bc":
        return B.BcConfig(obs_dim=od, act_dim=ad, policy_model_config=B.BcModelConfig(CandleMlpConfig(tuple(units["policy"]), "None"), opt("")), batch_size=bsz,
                          action_type="Continuous", device=0, seed=seed, kernel_form=extra)
    critic = MultiCriticConfig(2, CandleMlpConfig(tuple(units["critic"]), "None"), opt("critic"), h["critic_tau"])
    actor = GaussianActorConfig(CandleMlpConfig(tuple(units["actor"]), "None"), opt("actor"), min_log_std=-5.0, max_log_std=2.0, action_limit=ActionLimit.Clamp(),
                                kind=extra or "Mlp3")
    if kind == "iql":
        return IqlConfig(obs_dim=od, act_dim=ad, value_config=ValueConfig(CandleMlpConfig(tuple(units["value"]), "None"), opt("value")), critic_config=critic,
                         actor_config=actor, gamma=h["gamma"], tau_iql=h["tau_iql"], inv_lambda=h["inv_lambda"], exp_adv_max=h["exp_adv_max"], batch_size=bsz,
                         train=train, seed=seed, device=0)
    if kind == "awac":
        return B.AwacConfig(obs_dim=od, act_dim=ad, critic_config=critic, actor_config=actor, gamma=h["gamma"], inv_lambda=h["inv_lambda"],
                            exp_adv_max=h["exp_adv_max"], batch_size=bsz, train=train, seed=seed, device=0)
    ent = B.EntCoefMode.Auto(h["target_entropy"], h["ent_coef_lr"]) if "ent_coef_lr" in h else B.EntCoefMode.Fix(alpha)
    return B.CandleSacConfig(obs_dim=od, act_dim=ad, critic_config=critic, actor_config=actor, gamma=h["gamma"], ent_coef_mode=ent, batch_size=bsz, train=train,
                             seed=seed, device=0)


def rows(shape, seed, n=N_ROWS):
    od, ad = shape[0], shape[1]
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, od)).astype(np.float32), rng.uniform(-0.9, 0.9, (n, ad)).astype(np.float32),
            rng.standard_normal((n, od)).astype(np.float32), rng.standard_normal(n).astype(np.float32),
            (rng.random(n) < 0.1).astype(np.int8), np.zeros(n, np.int8))


def dataset(B, shape, seed=7):
    """a ring of capacity 128 holding 100 rows: the owner of the members' views"""
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=128, seed=seed), (shape[0],), np.float32, (shape[1],), np.float32, device=0)
    rb.push(*rows(shape, 1000 + seed))
    return rb


def own_batch(kind, shape, seed):
    r = rows(shape, 5000 + seed, shape[3])
    return r[:2] if kind == "bc" else r


def models(kind):
    """(model name or None for the default model, its roles) over everything the parameter views serve"""
    if kind == "bc":
        return [(None, ROLES)]
    out = [("actor", ROLES)] + [(f"critic_{i}", ROLES) for i in range(2)] + [(f"critic_tgt_{i}", ("param",)) for i in range(2)]
    return out + ([("value", ROLES)] if kind == "iql" else [("log_alpha", ROLES)] if kind == "candle_sac" else [])


def state(kind, agent):
    """every (model, role) of the agent's model table"""
    return {(m, r): agent.get_params(m, role=r) for m, roles in models(kind) for r in roles}


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def assert_same(got, want, tag):
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]), (tag, k)
