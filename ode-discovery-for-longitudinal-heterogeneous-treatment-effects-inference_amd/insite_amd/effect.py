"""Result container of the treatment-effect bands (include/insite_effect.h).

The hot path is ``ops.effect_bands``: per row and step, the trajectory under plan A, under plan B and their difference
A - B (paired within each bootstrap replicate), each with the point model's value and mean, standard deviation and
quantiles over the replicates 1..R-1.  This module only names the slices of its output.
"""
from __future__ import annotations

import dataclasses

import torch

SERIES = ("a", "b", "effect")


@dataclasses.dataclass
class EffectResult:
    """``series``: the names of the leading dimension, ("a",) or ("a", "b", "effect").  ``point``, ``mean``, ``std``
    [S, N, T]: the point model (replicate 0) and the mean / standard deviation (n - 1 divisor) over the replicates
    1..R-1; ``quantiles`` [S, Q, N, T] in the order of ``q``.  ``result["effect"]`` gives one series as a dict."""
    point: torch.Tensor
    mean: torch.Tensor
    std: torch.Tensor
    quantiles: torch.Tensor
    q: tuple
    series: tuple = SERIES

    def __getitem__(self, name: str) -> dict:
        i = self.series.index(name)
        return {"point": self.point[i], "mean": self.mean[i], "std": self.std[i], "quantiles": self.quantiles[i]}


def from_bands(out: torch.Tensor, q, shift: float = 0.0, scale: float = 1.0) -> EffectResult:
    """``ops.effect_bands``' out [S, 3 + Q, N, T] as an ``EffectResult`` in the scale (x - shift) / scale: locations of
    the series a and b are shifted and divided, their standard deviations and every statistic of the effect series
    (a difference: the shift cancels) are divided only."""
    S = out.size(0)
    if S not in (1, 3) or out.dim() != 4 or out.size(1) != 3 + len(q):
        raise ValueError("out must be [1 or 3, 3 + Q, N, T]")
    res = out / scale
    loc = [0, 1] + list(range(3, out.size(1)))      # point, mean and quantiles
    res[:min(S, 2), loc] = (out[:min(S, 2), loc] - shift) / scale
    return EffectResult(point=res[:, 0], mean=res[:, 1], std=res[:, 2], quantiles=res[:, 3:],
                        q=tuple(float(v) for v in q), series=SERIES[:S])


@dataclasses.dataclass
class CohortEffectResult:
    """The cohort / subgroup averages of ``ops.cohort_effect`` (include/insite_cohort.h).  ``series``:
    ("a",) or ("a", "b", "effect").  ``point``, ``mean``, ``std`` [S, G, T]: per group the point model's weighted mean
    trajectory and the mean / standard deviation (n - 1 divisor) of the replicates' weighted means; ``quantiles``
    [S, Q, G, T] in the order of ``q``; ``weight_sum`` [R, G]: the weight every replicate gave every group (0: the
    replicate drew no row of the group, and the group's statistics are NaN).  ``result["effect"]`` gives one series
    as a dict."""
    point: torch.Tensor
    mean: torch.Tensor
    std: torch.Tensor
    quantiles: torch.Tensor
    weight_sum: torch.Tensor
    q: tuple
    series: tuple = SERIES

    def __getitem__(self, name: str) -> dict:
        i = self.series.index(name)
        return {"point": self.point[i], "mean": self.mean[i], "std": self.std[i], "quantiles": self.quantiles[i]}


def from_cohort(out: torch.Tensor, wsum: torch.Tensor, q, shift: float = 0.0, scale: float = 1.0) -> CohortEffectResult:
    """``ops.cohort_effect``'s out [G, S, 3 + Q, T] and wsum [R, G] as a ``CohortEffectResult`` in the scale
    (x - shift) / scale, by ``from_bands``' rule: locations of the series a and b are shifted and divided, their
    standard deviations and every statistic of the effect series are divided only."""
    if out.dim() != 4 or out.size(1) not in (1, 3) or out.size(2) != 3 + len(q):
        raise ValueError("out must be [G, 1 or 3, 3 + Q, T]")
    S = out.size(1)
    o = out.permute(1, 2, 0, 3)                     # [S, 3 + Q, G, T]
    res = o / scale
    loc = [0, 1] + list(range(3, o.size(1)))        # point, mean and quantiles
    res[:min(S, 2), loc] = (o[:min(S, 2), loc] - shift) / scale
    return CohortEffectResult(point=res[:, 0], mean=res[:, 1], std=res[:, 2], quantiles=res[:, 3:], weight_sum=wsum,
                              q=tuple(float(v) for v in q), series=SERIES[:S])


REGIMEN_SERIES = ("value", "regret")


@dataclasses.dataclass
class RegimenChoiceResult:
    """The choice among K treatment plans of ``ops.regimen_choice`` (include/insite_regimen.h).
    ``choice`` int32 [N]: the point model's best plan (-1: the point model has a NaN objective); ``win`` [N, K]: the
    share of the replicates 1..R-1 in which plan j is the best (a row sums to 1 minus the share of replicates that
    abstain).  ``series``: ("value", "regret").  ``point``, ``mean``, ``std`` [2, N, K]: per plan the objective and the
    regret against the replicate's own best plan, as the point model's value and the mean / standard deviation (n - 1
    divisor) over the replicates 1..R-1; ``quantiles`` [2, Q, N, K] in the order of ``q``.  ``result["regret"]`` gives
    one series as a dict."""
    choice: torch.Tensor
    win: torch.Tensor
    point: torch.Tensor
    mean: torch.Tensor
    std: torch.Tensor
    quantiles: torch.Tensor
    q: tuple
    series: tuple = REGIMEN_SERIES

    def __getitem__(self, name: str) -> dict:
        i = self.series.index(name)
        return {"point": self.point[i], "mean": self.mean[i], "std": self.std[i], "quantiles": self.quantiles[i]}


def from_regimen(choice: torch.Tensor, win: torch.Tensor, out: torch.Tensor, q, shift=0.0,
                 scale: float = 1.0) -> RegimenChoiceResult:
    """``ops.regimen_choice``'s (choice, win, out [N, K, 2, 3 + Q]) as a ``RegimenChoiceResult`` in the scale
    (x - shift) / scale: the locations of the value series (point, mean, quantiles) are shifted and divided, its
    standard deviation and every statistic of the regret (a difference: the shift cancels) are divided only.
    ``shift``: a number or a tensor [N] (the shift of a weighted sum is the row's weight total times the mean)."""
    if out.dim() != 4 or out.size(2) != 2 or out.size(3) != 3 + len(q):
        raise ValueError("out must be [N, K, 2, 3 + Q]")
    o = out.permute(2, 3, 0, 1)                     # [2, 3 + Q, N, K]
    res = o / scale
    loc = [0, 1] + list(range(3, o.size(1)))        # point, mean and quantiles
    sh = shift[:, None] if isinstance(shift, torch.Tensor) else shift
    res[0, loc] = (o[0, loc] - sh) / scale
    return RegimenChoiceResult(choice=choice, win=win, point=res[:, 0], mean=res[:, 1], std=res[:, 2],
                               quantiles=res[:, 3:], q=tuple(float(v) for v in q))


FEEDBACK_SERIES = ("value", "regret", "exposure")


@dataclasses.dataclass
class ThresholdRule:
    """A closed-loop treatment rule on the predicted state (include/insite_feedback.h): every
    ``every``-th step, switch to ``arm_on`` when the state before the step is >= ``on`` and back to ``arm_off`` when
    it falls below ``off`` (``off`` None: ``off = on``, the memoryless rule; ``off < on``: hysteresis).  ``on`` and
    ``off`` are numbers or arrays [N] (one threshold per row), in the units of ``get_predictions``.  ``start_on``:
    the rule's flag before the first step (it matters only under hysteresis)."""
    on: object
    off: object = None
    arm_on: int = 1
    arm_off: int = 0
    every: int = 1
    start_on: bool = False


@dataclasses.dataclass
class FeedbackResult:
    """K closed-loop rules per row of ``ops.feedback_rules`` (include/insite_feedback.h).  ``choice``
    int32 [N]: the point model's best rule (-1: it has a NaN objective); ``win`` [N, K]: the share of the replicates
    1..R-1 in which rule j is the best.  ``series``: ("value", "regret", "exposure").  ``point``, ``mean``, ``std``
    [3, N, K]: per rule the objective, the regret against the replicate's own best rule and the exposure (the number
    of steps spent on), as the point model's value and the mean / standard deviation (n - 1 divisor) over the
    replicates 1..R-1; ``quantiles`` [3, Q, N, K] in the order of ``q``.  ``schedule`` int8 [N, K, T] or None: the arm
    the point model applies at every step under every rule.  ``result["exposure"]`` gives one series as a dict."""
    choice: torch.Tensor
    win: torch.Tensor
    point: torch.Tensor
    mean: torch.Tensor
    std: torch.Tensor
    quantiles: torch.Tensor
    q: tuple
    schedule: torch.Tensor | None = None
    series: tuple = FEEDBACK_SERIES

    def __getitem__(self, name: str) -> dict:
        i = self.series.index(name)
        return {"point": self.point[i], "mean": self.mean[i], "std": self.std[i], "quantiles": self.quantiles[i]}


def from_feedback(choice: torch.Tensor, win: torch.Tensor, out: torch.Tensor, q, schedule=None, shift=0.0,
                  scale: float = 1.0) -> FeedbackResult:
    """``ops.feedback_rules``' (choice, win, out [N, K, 3, 3 + Q], sched) as a ``FeedbackResult`` in the scale
    (x - shift) / scale, by ``from_regimen``'s rule: the locations of the value series are shifted and divided, its
    standard deviation and every statistic of the regret are divided only; the exposure (a count of steps) is left
    as it is.  ``shift``: a number or a tensor [N]."""
    if out.dim() != 4 or out.size(2) != 3 or out.size(3) != 3 + len(q):
        raise ValueError("out must be [N, K, 3, 3 + Q]")
    o = out.permute(2, 3, 0, 1)                     # [3, 3 + Q, N, K]
    res = o.clone()
    res[:2] = o[:2] / scale
    loc = [0, 1] + list(range(3, o.size(1)))        # point, mean and quantiles
    sh = shift[:, None] if isinstance(shift, torch.Tensor) else shift
    res[0, loc] = (o[0, loc] - sh) / scale
    return FeedbackResult(choice=choice, win=win, point=res[:, 0], mean=res[:, 1], std=res[:, 2],
                          quantiles=res[:, 3:], q=tuple(float(v) for v in q), schedule=schedule)


def policy_series(n_plans: int) -> tuple:
    """The names of the 2 K + 6 series of ``ops.policy_value`` in the order of include/insite_policy.h."""
    K = int(n_plans)
    return (tuple(f"value_{j}" for j in range(K))
            + ("personalised", "rule", "best_fixed", "gain_personalised", "gain_rule", "optimism")
            + tuple(f"share_{j}" for j in range(K)))


@dataclasses.dataclass
class PolicyValueResult:
    """The cohort value of a personalised choice among K plans of ``ops.policy_value`` (include/insite_policy.h,
    DESIGN.md §9k).  ``series``: ``policy_series(K)`` -- value_j (everyone gets plan j), personalised (every row its
    own best plan, re-derived inside each replicate), rule (the fixed per-row ``rule`` under each replicate's model),
    best_fixed (the best single plan of the replicate), gain_personalised = best_fixed - personalised, gain_rule =
    best_fixed - rule and optimism = rule - personalised (signed by the sense: the first and the last are >= 0, gain_rule
    is negative where the rule is worse than the best single plan), share_j (the weight share
    of the rows whose best plan is j).  ``point``, ``mean``, ``std`` [S, G]: per group the point model's value and the
    mean / standard deviation (n - 1 divisor) over the replicates 1..R-1; ``quantiles`` [S, Q, G] in the order of
    ``q``.  ``fixwin`` [G, K]: the share of the replicates in which plan j is the best fixed plan; ``best_fixed``
    int32 [G]: the point model's (-1: it has a NaN value); ``rule`` int32 [N]; ``weight_sum`` [R, G].
    ``result["optimism"]`` gives one series as a dict, ``result.share`` the K share series as [K, G] statistics."""
    point: torch.Tensor
    mean: torch.Tensor
    std: torch.Tensor
    quantiles: torch.Tensor
    fixwin: torch.Tensor
    best_fixed: torch.Tensor
    rule: torch.Tensor
    weight_sum: torch.Tensor
    q: tuple
    series: tuple
    n_plans: int

    def __getitem__(self, name: str) -> dict:
        i = self.series.index(name)
        return {"point": self.point[i], "mean": self.mean[i], "std": self.std[i], "quantiles": self.quantiles[i]}

    @property
    def share(self) -> dict:
        lo = self.n_plans + 6
        return {"point": self.point[lo:], "mean": self.mean[lo:], "std": self.std[lo:],
                "quantiles": self.quantiles[lo:].transpose(0, 1)}


def from_policy(out: torch.Tensor, fixwin: torch.Tensor, best_fixed: torch.Tensor, rule: torch.Tensor,
                wsum: torch.Tensor, q, shift: float = 0.0, scale: float = 1.0) -> PolicyValueResult:
    """``ops.policy_value``'s outputs as a ``PolicyValueResult`` in the scale (x - shift) / scale: the locations
    (point, mean, quantiles) of the value, personalised, rule and best_fixed series are shifted and divided, their
    standard deviations and every statistic of the three differences (the shift cancels) are divided only, the shares
    are left as they are.  ``shift``: the mean times the weight total of a row's steps."""
    if out.dim() != 3 or out.size(1) < 8 or out.size(1) % 2 or out.size(2) != 3 + len(q):
        raise ValueError("out must be [G, 2 K + 6, 3 + Q]")
    K = out.size(1) // 2 - 3
    o = out.permute(1, 2, 0)                        # [S, 3 + Q, G]
    res = o.clone()
    loc = [0, 1] + list(range(3, o.size(1)))        # point, mean and quantiles
    res[:K + 6] = o[:K + 6] / scale
    res[:K + 3, loc] = (o[:K + 3, loc] - shift) / scale
    return PolicyValueResult(point=res[:, 0], mean=res[:, 1], std=res[:, 2], quantiles=res[:, 3:], fixwin=fixwin,
                             best_fixed=best_fixed, rule=rule, weight_sum=wsum, q=tuple(float(v) for v in q),
                             series=policy_series(K), n_plans=K)


def rule_value_series(n_rules: int) -> tuple:
    """The names of the 3 K + 9 series of ``ops.rule_value`` in the order of include/insite_rulevalue.h."""
    K = int(n_rules)
    return (tuple(f"value_{j}" for j in range(K))
            + ("personalised", "assigned", "best_fixed", "gain_personalised", "gain_assigned", "optimism")
            + tuple(f"share_{j}" for j in range(K)) + tuple(f"exposure_{j}" for j in range(K))
            + ("exposure_personalised", "exposure_assigned", "exposure_best_fixed"))


@dataclasses.dataclass
class RuleValueResult:
    """The cohort value of K closed-loop rules of ``ops.rule_value`` (include/insite_rulevalue.h).
    ``series``: ``rule_value_series(K)`` -- value_j (everyone follows rule j), personalised (every row its own best
    rule, re-derived inside each replicate), assigned (the fixed per-row ``assign`` under each replicate's model),
    best_fixed (the best single rule of the replicate), gain_personalised = best_fixed - personalised, gain_assigned =
    best_fixed - assigned and optimism = assigned - personalised (signed by the sense: the first and the last are
    >= 0), share_j (the weight share of the rows whose best rule is j), exposure_j (the treated steps per row when
    everyone follows rule j), exposure_personalised, exposure_assigned and exposure_best_fixed.  ``point``, ``mean``,
    ``std`` [S, G]: per group the point model's value and the mean / standard deviation (n - 1 divisor) over the
    replicates 1..R-1; ``quantiles`` [S, Q, G] in the order of ``q``.  ``fixwin`` [G, K]: the share of the replicates
    in which rule j is the best fixed rule; ``best_fixed`` int32 [G]: the point model's (-1: it has a NaN value);
    ``assign`` int32 [N]; ``weight_sum`` [R, G].  ``result["optimism"]`` gives one series as a dict,
    ``result.share`` the K share series as [K, G] statistics, ``result.exposure`` the K + 3 exposure series as
    [K + 3, G] statistics."""
    point: torch.Tensor
    mean: torch.Tensor
    std: torch.Tensor
    quantiles: torch.Tensor
    fixwin: torch.Tensor
    best_fixed: torch.Tensor
    assign: torch.Tensor
    weight_sum: torch.Tensor
    q: tuple
    series: tuple
    n_rules: int

    def __getitem__(self, name: str) -> dict:
        i = self.series.index(name)
        return {"point": self.point[i], "mean": self.mean[i], "std": self.std[i], "quantiles": self.quantiles[i]}

    def _block(self, lo, hi) -> dict:
        return {"point": self.point[lo:hi], "mean": self.mean[lo:hi], "std": self.std[lo:hi],
                "quantiles": self.quantiles[lo:hi].transpose(0, 1)}

    @property
    def share(self) -> dict:
        return self._block(self.n_rules + 6, 2 * self.n_rules + 6)

    @property
    def exposure(self) -> dict:
        return self._block(2 * self.n_rules + 6, 3 * self.n_rules + 9)


def from_rule_value(out: torch.Tensor, fixwin: torch.Tensor, best_fixed: torch.Tensor, assign: torch.Tensor,
                    wsum: torch.Tensor, q, shift: float = 0.0, scale: float = 1.0) -> RuleValueResult:
    """``ops.rule_value``'s outputs as a ``RuleValueResult`` in the scale (x - shift) / scale, by ``from_policy``'s
    rule: the locations (point, mean, quantiles) of the value, personalised, assigned and best_fixed series are
    shifted and divided, their standard deviations and every statistic of the three differences (the shift cancels)
    are divided only, the shares and the exposures (counts of steps) are left as they are.  ``shift``: the mean times
    the weight total of a row's steps."""
    if out.dim() != 3 or out.size(1) < 12 or out.size(1) % 3 or out.size(2) != 3 + len(q):
        raise ValueError("out must be [G, 3 K + 9, 3 + Q]")
    K = out.size(1) // 3 - 3
    o = out.permute(1, 2, 0)                        # [S, 3 + Q, G]
    res = o.clone()
    loc = [0, 1] + list(range(3, o.size(1)))        # point, mean and quantiles
    res[:K + 6] = o[:K + 6] / scale
    res[:K + 3, loc] = (o[:K + 3, loc] - shift) / scale
    return RuleValueResult(point=res[:, 0], mean=res[:, 1], std=res[:, 2], quantiles=res[:, 3:], fixwin=fixwin,
                           best_fixed=best_fixed, assign=assign, weight_sum=wsum, q=tuple(float(v) for v in q),
                           series=rule_value_series(K), n_rules=K)


@dataclasses.dataclass
class EnsembleScore:
    """The bootstrap ensemble scored against observed outcomes (``ops.ensemble_score``, include/insite_score.h,
    DESIGN.md §9p), per group and step.  ``n``, ``n_bad`` [G, T]: the scored cells and the observed cells with a
    non-finite replicate; ``rmse_point``, ``rmse_mean``: of the point model and of the ensemble mean; ``spread`` =
    sqrt(mean ensemble variance) (calibrated against ``rmse_mean``: under-dispersed when smaller); ``crps``: the mean
    CRPS of the ensemble's empirical distribution; ``coverage``, ``width``, ``interval_score`` [G, L, T]: of the
    central bands of ``levels``; ``pit_hist`` [G, B, T]: the rank histogram as frequencies.  ``pooled``: the same
    names without the step dimension, from the sums added over the steps first.  A cell count of 0 gives NaN.
    ``sums``: the additive sums all of it was made from."""
    n: torch.Tensor
    n_bad: torch.Tensor
    rmse_point: torch.Tensor
    rmse_mean: torch.Tensor
    spread: torch.Tensor
    crps: torch.Tensor
    coverage: torch.Tensor
    width: torch.Tensor
    interval_score: torch.Tensor
    pit_hist: torch.Tensor
    pooled: dict
    sums: torch.Tensor
    levels: tuple
    n_bins: int
    scale: float = 1.0

    def merge(self, other: "EnsembleScore") -> "EnsembleScore":
        """The score of the union of two shards: their sums added (equal levels, bins, scale and shape)."""
        if (self.levels != other.levels or self.n_bins != other.n_bins or self.scale != other.scale
                or self.sums.shape != other.sums.shape):
            raise ValueError("merge needs scores of equal levels, bins, scale and shape")
        return from_score(self.sums + other.sums.to(self.sums.device), self.levels, self.n_bins, self.scale)


def _score_stats(s: torch.Tensor, L: int, B: int, scale: float) -> dict:
    """s [G, S, ...] -> the statistics over the trailing dimensions (a cell count of 0: 0 / 0 = NaN)."""
    n = s[:, 0]
    lv = s[:, 6 + B:].reshape((s.size(0), L, 3) + tuple(s.shape[2:]))
    nl = n[:, None]
    return {
        "n": n, "n_bad": s[:, 1],
        "rmse_point": torch.sqrt(s[:, 2] / n) / scale,
        "rmse_mean": torch.sqrt(s[:, 3] / n) / scale,
        "spread": torch.sqrt(s[:, 4] / n) / scale,
        "crps": s[:, 5] / n / scale,
        "pit_hist": s[:, 6:6 + B] / nl,
        "coverage": lv[:, :, 0] / nl,
        "width": lv[:, :, 1] / nl / scale,
        "interval_score": lv[:, :, 2] / nl / scale,
    }


def from_score(sums: torch.Tensor, levels, n_bins: int, scale: float = 1.0) -> EnsembleScore:
    """``ops.ensemble_score``'s sums [G, 6 + B + 3 L, T] as an ``EnsembleScore`` in the scale x / scale: lengths
    (RMSE, spread, CRPS, width, interval score) are divided by ``scale`` -- the squared sums by its square --, counts
    and frequencies are left as they are.  The pooled figures add the sums over the steps first and divide after."""
    levels = tuple(float(v) for v in levels)
    L, B = len(levels), int(n_bins)
    if sums.dim() != 3 or sums.size(1) != 6 + B + 3 * L:
        raise ValueError("sums must be [G, 6 + n_bins + 3 n_levels, T]")
    per = _score_stats(sums, L, B, float(scale))
    pooled = _score_stats(sums.sum(dim=2), L, B, float(scale))
    return EnsembleScore(pooled=pooled, sums=sums, levels=levels, n_bins=B, scale=float(scale), **per)
