"""Independent restatement of border-candle-agent's Bc::opt_ (bc/base.rs:167-198) in float32 PyTorch autograd on the CPU: the checker of
the HIP BC agent.  Nothing under border_amd/ imports this file.

  policy      Mlp (mlp/base.rs, mlp.rs:14-24): x @ W.T + b per layer, ReLU after every layer but the last, activation_out
              (None | ReLU | Tanh | Sigmoid, lib.rs:58-74) after the last
  opt_        loss = mse(policy(obs), act) = the mean of the squared differences over all B x A elements (candle_nn::loss::mse);
              backward_step; the record's one key is "loss".  BcActionType::Discrete panics (:174)
  sample      Continuous: the network output; Discrete: argmax over the last dimension as i64 (:49-59)
  optimizer   the Adam / AdamW element formulas of tests/iql_restatement.py (AdamState), no gradient clipping

Parameters travel in the agent's reference layout: per layer ln{k}.weight [out][in] then ln{k}.bias [out].
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np
import torch

from iql_restatement import AdamState, Mlp, init_flat, mlp_count

ACT_OUT = {"None": lambda x: x, "ReLU": torch.relu, "Tanh": torch.tanh, "Sigmoid": torch.sigmoid}


@dataclass
class BcSpec:
    obs_dim: int
    act_dim: int
    units: Sequence[int] = (256, 256)
    activation_out: str = "None"
    lr: float = 1e-3
    adamw: Optional[dict] = None          # None: Adam{lr}; else AdamW kwargs (beta1, beta2, eps, wd)
    action_type: str = "Continuous"

    def count(self) -> int:
        return mlp_count(self.obs_dim, self.units, self.act_dim)

    def init_params(self, seed: int) -> np.ndarray:
        return init_flat(self.obs_dim, self.units, self.act_dim, np.random.default_rng(seed))

    def to_config(self, B, batch_size: int, device: Optional[int] = None, seed: int = 0, kernel_form: str = "default", head_rows: int = 0):
        opt = B.OptimizerConfig.Adam(self.lr) if self.adamw is None else B.OptimizerConfig.AdamW(
            self.lr, self.adamw["beta1"], self.adamw["beta2"], self.adamw["wd"], self.adamw["eps"])
        return B.BcConfig(obs_dim=self.obs_dim, act_dim=self.act_dim,
                          policy_model_config=B.BcModelConfig(B.CandleMlpConfig(tuple(self.units), self.activation_out), opt),
                          batch_size=batch_size, action_type=self.action_type, device=device, seed=seed, kernel_form=kernel_form,
                          head_rows=head_rows)


def make_batch(spec: BcSpec, n: int, seed: int):
    """obs ~ N(0, 1); actions inside the range of the output activation, so that every activation has something to fit"""
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((n, spec.obs_dim)).astype(np.float32)
    lo, hi = {"None": (-1.0, 1.0), "ReLU": (-0.2, 1.0), "Tanh": (-0.95, 0.95), "Sigmoid": (0.05, 0.95)}[spec.activation_out]
    act = rng.uniform(lo, hi, (n, spec.act_dim)).astype(np.float32)
    return obs, act


class BcRestatement:
    def __init__(self, spec: BcSpec, flat: np.ndarray):
        self.spec = spec
        self.net = Mlp(spec.obs_dim, spec.units, spec.act_dim, False, flat)   # the last layer's activation is applied in forward()
        kw = {} if spec.adamw is None else spec.adamw
        self.opt = AdamState(self.net.params, spec.lr, adamw=spec.adamw is not None, **kw)
        self.probes = {}

    def forward(self, obs) -> torch.Tensor:
        return ACT_OUT[self.spec.activation_out](self.net.forward(torch.as_tensor(np.asarray(obs, np.float32))))

    def update(self, obs, act) -> dict:
        if self.spec.action_type == "Discrete":
            raise RuntimeError("Bc::opt_ panics for BcActionType::Discrete (bc/base.rs:174)")
        for p in self.net.params:
            p.grad = None
        z = self.net.forward(torch.as_tensor(np.asarray(obs, np.float32)))
        z.retain_grad()
        pred = ACT_OUT[self.spec.activation_out](z)
        d = pred - torch.as_tensor(np.asarray(act, np.float32))
        loss = (d * d).mean()          # over all B x A elements
        loss.backward()
        self.probes = {"pred": pred.detach().numpy().copy(), "dz": z.grad.numpy().copy(), "grad": self.net.flat(grad=True)}
        self.opt.step()
        return {"loss": float(loss.detach())}

    def params(self) -> np.ndarray:
        return self.net.flat()

    @torch.no_grad()
    def sample(self, obs) -> np.ndarray:
        y = self.forward(obs)
        if self.spec.action_type == "Discrete":
            return y.argmax(dim=-1).numpy().astype(np.int64)
        return y.numpy()
