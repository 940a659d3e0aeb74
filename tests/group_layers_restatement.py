"""A Python restatement of which step an Mlp DQN agent takes (DqnMlp::fused_ok, border_amd/csrc/mlp_agents.hip) and of the launches
DqnMlp::update_critic enqueues for one update on its latency-shaped layer path behind the gather of replay_sample_on_stream - written
from those two functions, not from border_amd/csrc/group_layers_plan.hpp, which tests/test_group_layers_host.py checks against it."""


def pad64(x):
    return (x + 63) // 64 * 64


class Shape:
    def __init__(self, in_dim, units, out_dim, batch, double_dqn=False, head_fuse=True):
        self.in_dim, self.units, self.out_dim, self.batch, self.double_dqn, self.head_fuse = in_dim, tuple(units), out_dim, batch, double_dqn, head_fuse
        widths = (in_dim,) + self.units + (out_dim,)
        self.Kp = [pad64(w) for w in widths[:-1]]
        self.Np = [pad64(w) for w in widths[1:]]
        self.L = len(self.Np)
        self.nz = 3 if double_dqn else 2


SHAPES = {   # the issue's shapes (a)-(d) and BASELINE config 1 (C1)
    "a": Shape(4, (64, 64), 2, 65),
    "b": Shape(4, (64, 64), 2, 65, double_dqn=True),
    "c": Shape(6, (64, 192), 5, 33),
    "d": Shape(4, (256, 256), 2, 64),
    "c1": Shape(4, (64, 64), 2, 64),
}


def fused_ok(s):
    """DqnMlp::fused_ok with the one-workgroup step switched on"""
    if s.L > 4 or s.batch > 128 or s.out_dim > 64:
        return False
    if any(k > 256 or n > 256 for k, n in zip(s.Kp, s.Np)):
        return False
    rb = (s.batch + 31) // 32
    return all(s.nz * rb * (n // 32) <= 8 and rb * (k // 32) * (n // 32) <= 8 for k, n in zip(s.Kp, s.Np))


def head_fused(s):
    """update_critic's head_fused on a uniform ring"""
    return s.head_fuse and s.L >= 2 and s.out_dim <= 32 and s.Kp[-1] <= 128


def launches(s, P=1):
    """[(kernel, grid x, y, z, threads)] of one update of P members: update_critic's launches for ONE member, with the member index as
    grid y (z for the row-block head, whose grid already has x and y; the layers keep the network instance in z)"""
    B, L, nz, rb = s.batch, s.L, s.nz, (s.batch + 31) // 32
    obs_bytes = 4 * s.in_dim
    nvec = obs_bytes // 16 if obs_bytes % 16 == 0 else obs_bytes // 4
    chunks = max(1, (nvec + 1023) // 1024)
    out = [("gather", B * chunks, P, 1, 256), ("pack", (nz * B * s.in_dim + 255) // 256, P, 1, 256)]
    head = head_fused(s)
    for i in range(L - 1 if head else L):
        out.append(("fwd", rb * (s.Np[i] // 32), P, nz, 256))
    if head:
        out.append(("head_td", rb, s.Kp[-1] // 64, P, 512))
    else:
        out += [("td_dense", (B + 3) // 4, P, 1, 256), ("mean_rows", 1, P, 1, 256)]
    for i in range(L - 2 if head else L - 1, 0, -1):
        out.append(("dx", rb * (s.Kp[i] // 32), P, 1, 256))
    chunks_dw = max(1, min(16, B // 256))
    out.append(("dw", sum((k // 32) * (n // 32) * chunks_dw for k, n in zip(s.Kp, s.Np)), P, 1, 256))
    total = sum(k * n + n for k, n in zip(s.Kp, s.Np))
    out.append(("reduce_adam", (total // 4 + 255) // 256, P, 1, 256))
    return out
