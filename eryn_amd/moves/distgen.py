"""HIP-backed ``DistributionGenerate`` (distgen.py:10-104): the independence proposal - every walker is proposed a fresh point
from a ``ProbDistContainer`` and carries the Hastings factor ``+logq(old) - logq(new)`` - with the reference's plugin contract,
``MHMove.propose`` (mh.py:56-193) over ``DistributionGenerate.get_proposal`` (distgen.py:34-104) for the single-branch
``nleaves_max == 1`` case.

``rng="numpy"``: the points come from the container's ``rvs`` on the global stream (distgen.py:97, prior.py:472-493) and the accept
uniforms from ``model.random`` (mh.py:157), in the reference's order; both log-densities, the factor, the prior, the likelihood,
the tempered accept test and the update run in libhipensemble (``hens_dist_step``, csrc/hens_dist.h).  With the same seeds the
chain is the reference's.  ``rng="philox"``: the launch draws the points itself (``hens_set_dist_proposal`` + ``hens_step``).
"""
import numpy as np

from ..prior import ProbDistContainer, prior_spec
from .device import mh_slot_key
from .gaussian import MHMove

__all__ = ["DistributionGenerate"]


class DistributionGenerate(MHMove):
    """``DistributionGenerate(generate_dist)``: ``generate_dist`` is ``{branch_name: container}`` with ``container`` an
    ``eryn_amd.prior.ProbDistContainer`` (or any container that carries ``priors_in``, ``rvs`` and ``logpdf`` the way the
    reference's does) or the ``{index: distribution}`` dict it is made of; uniform, log-uniform and normal entries."""

    def __init__(self, generate_dist, **kwargs):
        if kwargs.get("gibbs_sampling_setup") is not None:
            raise NotImplementedError("DistributionGenerate(gibbs_sampling_setup=...) is not built: the device draws whole rows from the "
                                      "generator (Gibbs blocks: eryn_amd.moves.StretchMove, GaussianMove)")
        if not isinstance(generate_dist, dict):                            # distgen.py:21-24
            raise ValueError(
                "When entering directly into the DistributionGenerate class, generate_dist must be a dictionary. The keys are branch names and the items are ProbDistContainer objects."
            )
        containers = {}
        for key, dist in generate_dist.items():                            # distgen.py:26-30
            if isinstance(dist, dict):
                dist = ProbDistContainer(dist)
            elif not isinstance(dist, ProbDistContainer) and not all(hasattr(dist, a) for a in ("priors_in", "rvs", "logpdf")):
                raise ValueError("Distributions need to be eryn.prior.ProbDistContainer object.")
            containers[key] = dist
        if len(containers) != 1:
            raise NotImplementedError("the device path handles a single branch")
        self.generate_dist = containers
        (self.branch_name, self.container), = containers.items()
        # the terms the device reads: the container itself, or a foreign container through the dict it was made of
        self.spec = prior_spec(self.container if isinstance(self.container, ProbDistContainer) else dict(self.container.priors_in))
        MHMove.__init__(self, **kwargs)

    def device_proposal(self):
        """("dist", prior_terms dict) for the context's MH slot (``HipEnsemble.set_dist_proposal``)."""
        return "dist", self.spec.terms

    def propose(self, model, state):
        name, br, T, W, D = self._single_branch(state)
        if self.spec.lo.shape != (D,):
            raise ValueError(f"generate_dist describes {self.spec.lo.shape[0]} parameters, the state has {D}")
        eng = self._ensure_engine(T, W, D)
        if hasattr(eng.likelihood, "evaluate"):
            raise NotImplementedError("MH moves on the device need a device likelihood")
        if self.rng == "philox":                                       # device-side draws (k_dist)
            return self._propose_philox(model, state, mh_proposal=self.device_proposal())
        self._upload_if_needed(eng, state, br)
        want = ("mh",) + mh_slot_key(self.device_proposal())
        if getattr(eng, "_move_cfg", None) != want:                    # (the slot may hold another move of the mix)
            eng.set_dist_proposal(self.spec.terms, 1.0)
            eng._move_cfg = want
        self._bump(eng)
        q = np.asarray(self.container.rvs(size=T * W), dtype=np.float64).reshape(T, W, D)     # distgen.py:97 (all leaves active)
        u_acc = model.random.rand(T, W)                                # mh.py:157
        accepted = eng.dist_step(q, u_acc)
        if self._accepted is not None:
            self.accepted += accepted                                  # mh.py:186
        self.num_proposals += 1
        return self._finish(eng, state, name, br, T, W), accepted

