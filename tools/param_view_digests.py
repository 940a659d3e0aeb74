"""Checkpoint digests of the ten agent forms, each built at the smallest size its constructor accepts.

Every model of a form is filled through the public set_params from numpy.random.default_rng(<the model's `which` id>), the agent is
saved in both checkpoint formats, and the program prints - as one JSON object - per form and format the written file names with
each file's SHA-256.  The bytes depend only on the values set and on the container code (the archive writer stamps time and date
as zero), so the digests are reproducible; tests/golden/param_view_digests.json holds the output of a run at the commit BEFORE the
model table and is never regenerated from the code under test.  tests/test_gpu_param_views.py imports FORMS, views() and the
helpers below.

    python tools/param_view_digests.py [out.json]
"""
import hashlib
import inspect
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FORMATS = ("tch", "safetensors")
TCH_MODELS = ("exp_avg", "exp_avg_sq", "grad")       # the tch DQN / IQN name their optimizer arenas as models 2, 3, 4
ROLES = ("param", "grad", "exp_avg", "exp_avg_sq")


def _candle(B, units=(5,), kind="Mlp3"):
    mlp = lambda: B.CandleMlpConfig(units=units)
    return dict(obs_dim=3, act_dim=2, actor_config=B.GaussianActorConfig(policy_config=mlp(), kind=kind),
                critic_config=B.MultiCriticConfig(n_nets=2, q_config=mlp()), batch_size=2, device=0)


def _forms():
    import border_amd as B
    adam = B.OptimizerConfig.Adam(1e-3)
    dqn = lambda q: B.Dqn(B.DqnConfig(model_config=B.DqnModelConfig(q_config=q, opt_config=adam), device=0))
    return {
        "dqn_cnn": lambda: dqn(B.AtariCnnConfig(n_stack=1, out_dim=3)),
        "dqn_mlp": lambda: dqn(B.MlpConfig(in_dim=3, units=(5,), out_dim=2)),
        "iqn_cnn": lambda: B.Iqn(B.IqnConfig(f_config=B.AtariCnnConfig(n_stack=1, skip_linear=True), feature_dim=3136, embed_dim=4, m_units=(5,),
                                             n_actions=3, device=0)),
        "iqn_mlp": lambda: B.Iqn(B.IqnConfig(f_config=B.MlpConfig(in_dim=3, units=(5,), out_dim=6), feature_dim=6, embed_dim=4, m_units=(5,),
                                             n_actions=2, device=0)),
        "sac": lambda: B.Sac(B.SacConfig(obs_dim=3, act_dim=2, pi_units=(5,), q_units=(5,), n_critics=2, ent_coef_mode=("Auto", -2.0, 3e-4),
                                         device=0)),
        "iql": lambda: B.Iql(B.IqlConfig(value_config=B.ValueConfig(value_config=B.CandleMlpConfig(units=(5,))), **_candle(B))),
        "awac": lambda: B.Awac(B.AwacConfig(**_candle(B))),
        "candle_sac_mlp2": lambda: B.CandleSac(B.CandleSacConfig(**_candle(B, units=(5, 5), kind="Mlp2"))),
        "bc": lambda: B.Bc(B.BcConfig(obs_dim=3, act_dim=2, policy_model_config=B.BcModelConfig(policy_model_config=B.CandleMlpConfig(units=(5,))),
                                      device=0)),
        "candle_dqn_mlp": lambda: B.CandleDqn(B.CandleDqnConfig(obs_dim=3, n_actions=2, device=0,
                                                                model_config=B.CandleDqnModelConfig(q_config=B.CandleMlpConfig(units=(5,))))),
        "candle_dqn_cnn": lambda: B.CandleDqn(B.CandleDqnConfig(q_config=B.AtariCnnConfig(n_stack=1, out_dim=3), device=0)),
    }


FORMS = ("dqn_cnn", "dqn_mlp", "iqn_cnn", "iqn_mlp", "sac", "iql", "awac", "candle_sac_mlp2", "bc", "candle_dqn_mlp", "candle_dqn_cnn")
DISCRETE = {"dqn_cnn": 3, "dqn_mlp": 2, "iqn_cnn": 3, "iqn_mlp": 2, "candle_dqn_mlp": 2, "candle_dqn_cnn": 3}   # form -> action count
CANDLE_CRITICS = ("iql", "awac", "candle_sac_mlp2")   # critic.tgt is saved from, and loaded into, the online critics


def build(form):
    return _forms()[form]()


class View:
    """One (model, role) of an agent behind the public get_params / set_params of its class."""

    def __init__(self, agent, model, role="param", saved=False):
        self.agent, self.model, self.role, self.saved = agent, model, role, saved
        by_which = "which" in inspect.signature(agent.get_params).parameters     # the tch Dqn and Iqn: get_params(which=<model>), no roles
        self.kw = {"which": model} if by_which else {"name": model, "role": role}
        self.id = agent.WHICH[model] if by_which else agent.which(model, role)
        self.label = model if role == "param" else f"{model}.{role}"

    def get(self):
        return self.agent.get_params(**self.kw)

    def set(self, values):
        self.agent.set_params(values, **self.kw)

    def values(self, n):
        return np.random.default_rng(self.id).standard_normal(n, dtype=np.float32)


def views(form, agent):
    """Every (model, role) the form exposes; .saved: the view's parameters are written by save_params and read back by load_params"""
    V = lambda *a, **k: View(agent, *a, **k)
    if form.startswith("dqn_"):
        return [V("qnet", saved=True), V("qnet_tgt", saved=True)] + [V(m) for m in TCH_MODELS]
    if form.startswith("iqn_"):
        return [V("iqn", saved=True), V("iqn_tgt", saved=True)] + [V(m) for m in TCH_MODELS]
    if form == "bc":
        return [V("policy", r, saved=r == "param") for r in ROLES]
    if form.startswith("candle_dqn_"):
        return [V("qnet", saved=True), V("qnet_tgt", saved=True)] + [V("qnet", r) for r in ROLES[1:]]
    if form == "sac":
        out = [V("pi", r, saved=r == "param") for r in ROLES]
        for i in range(2):
            out += [V(f"qnet_{i}", r, saved=r == "param") for r in ROLES] + [V(f"qnet_tgt_{i}", saved=True)]
        return out + [V("log_alpha", saved=True), V("log_alpha", "exp_avg"), V("log_alpha", "exp_avg_sq")]
    out = [V("actor", r, saved=r == "param") for r in ROLES]
    for i in range(2):
        out += [V(f"critic_{i}", r, saved=r == "param") for r in ROLES] + [V(f"critic_tgt_{i}")]     # the targets are in no file
    if form == "iql":
        out += [V("value", r, saved=r == "param") for r in ROLES]
    if form == "candle_sac_mlp2":
        out += [V("log_alpha", r, saved=r == "param") for r in ROLES]
    return out


def fill(vs):
    """sets every view from its generator; -> {label: the values set}"""
    vals = {}
    for v in vs:
        vals[v.label] = v.values(v.get().size)
        v.set(vals[v.label])
    return vals


def save_digests(agent, directory):
    """-> {format: [[file name, sha256], ...]} in the order save_params returns the files"""
    out = {}
    for fmt in FORMATS:
        agent.set_checkpoint_format(fmt)
        d = os.path.join(directory, fmt)
        out[fmt] = [[os.path.basename(f), hashlib.sha256(open(f, "rb").read()).hexdigest()] for f in agent.save_params(d)]
    return out


def main():
    res = {}
    for form in FORMS:
        agent = build(form)
        fill(views(form, agent))
        with tempfile.TemporaryDirectory() as d:
            res[form] = save_digests(agent, d)
        agent.close()
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
