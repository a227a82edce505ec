"""deepgroebner_amd — MI355X-native BuchbergerEnv step path (drop-in for deepgroebner's
LeadMonomialsEnv / CLeadMonomialsEnv and its ideal generators)."""
from .buchberger import (BuchbergerAgent, BuchbergerEnv, CLeadMonomialsEnv, LeadMonomialsAgent, LeadMonomialsEnv,  # noqa: F401
                         LookaheadAgent, PolyLists, VecLeadMonomialsEnv, buchberger, interreduce, lead_monomials_vector,
                         minimalize, reduce, reduce_many, select, spoly, spoly_many, strategy_stats, update)
from .ideals import (FixedIdealGenerator, RandomBinomialIdealGenerator, RandomIdealGenerator,  # noqa: F401
                     basis, cyclic, degree_distribution, format_ideal, parse_ideal_dist, parse_ideal_string,
                     parse_polynomial)

# the consumer side (deepgroebner_amd.rollout: policy, critic, trajectory buffer, rollout and update loops) needs torch, which the
# environment classes above do not: its names resolve here on first use
_ROLLOUT = ("PMLPPolicy", "PMLPValue", "DeviceTrajectoryBuffer", "run_rollout", "run_rollout_fused", "ppo_update", "value_update",
            "evaluate_policy", "episode_returns")


def __getattr__(name):
    if name in _ROLLOUT:
        from . import rollout
        return getattr(rollout, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
