"""Population-based training over a group of dense agents (BcGroup, IqlGroup, AwacGroup, CandleSacGroup): the selection rule on the
host in numpy, the work in the group's own calls - `train_offline` (the compiled loop), `evaluate` (lockstep), `copy_members` (exploit:
one launch, csrc/group_copy.hpp) and `set_hyper` (explore).  No compiled loop of its own.

    sched = TruncationSelection(frac=0.25, factors=(0.8, 1.25), names=("lr_actor", "lr_critic"), bounds={"lr_actor": (1e-5, 1e-2)}, seed=0)
    history = run_offline(group, views, evaluators, total_opts=100_000, interval=5_000, schedule=sched)

Successive halving is the same loop with `factors=(1.0,)`; a learning-rate schedule is `set_hyper` alone."""
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np


def rank(scores) -> np.ndarray:
    """member indices from the best score to the worst: higher is better, equal scores in member order, NaN last"""
    s = np.asarray(scores, np.float64).reshape(-1)
    key = np.where(np.isnan(s), -np.inf, s)
    order = np.argsort(-key, kind="stable")
    return np.concatenate([order[~np.isnan(s[order])], order[np.isnan(s[order])]])


class TruncationSelection:
    """Truncation selection with multiplicative perturbation: each member of the bottom `frac` of the population takes the state and
    the hyperparameters of a member drawn uniformly from the top `frac`, every hyperparameter of `names` multiplied by a factor drawn
    uniformly from `factors` and clipped to `bounds[name]` = (low, high) where given.  k = floor(frac * P), at most P // 2, members
    change hands: top and bottom never overlap, so no member is both a source and a destination and no destination appears twice
    (what `copy_members` requires).  A member whose score is NaN ranks last and is never a source.  Pure numpy, deterministic in
    `seed`: the n-th `step` of two objects built alike returns the same pairs and values for the same arguments."""

    def __init__(self, frac: float = 0.25, factors: Sequence[float] = (0.8, 1.25), names: Sequence[str] = (), bounds: Optional[Dict[str, Tuple[float, float]]] = None,
                 seed: int = 0):
        if not 0.0 <= frac <= 0.5:
            raise ValueError(f"frac must lie in [0, 0.5], got {frac}")
        if len(factors) == 0 or any(not np.isfinite(f) or f <= 0 for f in factors):
            raise ValueError("factors must be positive numbers")
        self.frac, self.factors, self.names = float(frac), tuple(float(f) for f in factors), tuple(names)
        self.bounds = dict(bounds or {})
        for n, (lo, hi) in self.bounds.items():
            if not lo <= hi:
                raise ValueError(f"bounds[{n!r}]: low {lo} exceeds high {hi}")
        self._rng = np.random.default_rng(seed)

    def step(self, scores, hypers: Dict[str, Sequence[float]]):
        """scores: one per member.  hypers: name -> one value per member, for every name of `names`.  Returns (pairs, values): pairs =
        [(source, destination), ...] in the order of the destinations' ranks (worst last), values = name -> float64 array of one
        value per member - a destination's is its source's, perturbed and clipped; everybody else's is what came in."""
        s = np.asarray(scores, np.float64).reshape(-1)
        P = s.size
        values = {n: np.array(hypers[n], np.float64).reshape(-1) for n in self.names}
        for n, v in values.items():
            if v.size != P:
                raise ValueError(f"hypers[{n!r}] holds {v.size} values for {P} members")
        k = min(int(self.frac * P), P // 2)
        order = rank(s)
        top = [int(i) for i in order[:k] if not np.isnan(s[i])]
        if k == 0 or not top:
            return [], values
        pairs = []
        for dst in order[P - k:]:
            src = top[int(self._rng.integers(len(top)))]
            pairs.append((src, int(dst)))
            for n in self.names:
                v = values[n][src] * self.factors[int(self._rng.integers(len(self.factors)))]
                if n in self.bounds:
                    v = min(max(v, self.bounds[n][0]), self.bounds[n][1])
                values[n][dst] = v
        return pairs, values


def run_offline(group, buffers, evaluators, total_opts: int, interval: int, schedule, on_generation=None) -> List[dict]:
    """Offline population-based training of `group` on `buffers` (one per member: views of one dataset will do): `interval` update
    rounds (`group.train_offline`), a lockstep evaluation (`group.evaluate(evaluators)`: one Evaluator per member), then
    `schedule.step(scores, hypers)` (a TruncationSelection, or anything with its `names` and `step`), `group.copy_members(pairs,
    hyper=True)` and `group.set_hyper` of every destination's new values - until total_opts rounds have run; the last generation is
    evaluated and not followed by a selection.  Returns the history, one dict per generation: {"opt_steps", "scores", "hypers" (name ->
    list, as trained with), "pairs", "set" (name -> {destination: value})}; on_generation(entry) sees each as it is made."""
    if interval < 1 or total_opts < 1:
        raise ValueError("total_opts and interval are positive")
    P, names = len(group), tuple(schedule.names)
    history, done = [], 0
    while done < total_opts:
        n = min(interval, total_opts - done)
        group.train_offline(buffers, n)
        done += n
        scores = [float(r.score) for r in group.evaluate(evaluators)]
        hypers = {name: [group.get_hyper(i, name) for i in range(P)] for name in names}
        entry = {"opt_steps": done, "scores": scores, "hypers": hypers, "pairs": [], "set": {name: {} for name in names}}
        if done < total_opts:
            pairs, values = schedule.step(scores, hypers)
            group.copy_members(pairs, hyper=True)
            for _, dst in pairs:
                for name in names:
                    group.set_hyper(dst, name, float(values[name][dst]))
                    entry["set"][name][dst] = float(values[name][dst])
            entry["pairs"] = [(int(s), int(d)) for s, d in pairs]
        history.append(entry)
        if on_generation is not None:
            on_generation(entry)
    return history
