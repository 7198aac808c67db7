"""HIP-backed ``MTDistGenMove`` (mtdistgen.py:7-136 over multipletry.py:62-594): the multiple-try independence proposal - every
walker is offered ``num_try`` fresh points from a ``ProbDistContainer``, one is picked with probability proportional to its
importance weight ``exp(beta logl + logp - logq)`` and the accept test compares the sum of the tries' weights with the sum in which
the current point stands in the picked try's place - with the reference's plugin contract, ``MHMove.propose`` (mh.py:56-193) over
``MultipleTryMove.get_proposal`` (multipletry.py:516-594) for the single-branch ``nleaves_max == 1`` case.

``rng="numpy"``: the tries come from ONE ``rvs(size=(T W, num_try))`` of the container and the pick uniforms from ONE
``np.random.rand(T W)``, both on the global stream (mtdistgen.py:70, multipletry.py:57), the accept uniforms from ``model.random``
(mh.py:157), in the reference's order; the log-densities, priors, likelihoods, both log-sum-exps, the pick, the factor, the
tempered accept test and the update run in libhipensemble (``hens_mt_dist_step``, csrc/hens_mt.h).  With the same seeds the chain
is the reference's.  ``rng="philox"``: the launch draws everything itself (``hens_set_mt_dist_proposal`` + ``hens_step``).
"""
import numbers

import numpy as np

from ..prior import ProbDistContainer, prior_spec
from .device import mh_slot_key
from .gaussian import MHMove

__all__ = ["MTDistGenMove"]

MAX_TRY = 64        # one tile row per try (csrc/hens_mt.h)


class MTDistGenMove(MHMove):
    """``MTDistGenMove(generate_dist, num_try=25, independent=True)``: ``generate_dist`` is a ``ProbDistContainer`` (what the
    reference's own test passes; or any container that carries ``priors_in``, ``rvs`` and ``logpdf`` the way the reference's does),
    ``{branch_name: container}`` or the ``{index: distribution}`` dict a container is made of; uniform, log-uniform and normal
    entries.  ``num_try`` is 1 .. 64.

    Only ``independent=True`` is built.  The reference's default ``independent=False`` raises ``UnboundLocalError`` inside
    ``get_mt_proposal`` (multipletry.py:456 reads a name only the independent branch assigns), so no chain depends on it.
    ``symmetric=True`` and ``gibbs_sampling_setup`` are not built; ``rj=True`` is ``eryn_amd.rj.MTDistGenMoveRJ``, a move of the
    leaf-packing sampler.

    An untempered sampler steps with beta = 1.  This is beyond the reference, whose move reads ``temperature_control.betas`` and
    raises without one.

    After ``propose()`` under ``rng="numpy"`` the move carries ``log_sum_weights`` and ``aux_log_sum_weights`` ``[T W]`` as the
    reference's does (multipletry.py:490-491)."""

    def __init__(self, generate_dist, num_try=1, independent=False, symmetric=False, rj=False, **kwargs):
        if kwargs.get("gibbs_sampling_setup") is not None:
            raise NotImplementedError("MTDistGenMove(gibbs_sampling_setup=...) is not built: the device draws whole rows from the "
                                      "generator (Gibbs blocks: eryn_amd.moves.StretchMove, GaussianMove)")
        if rj:
            raise NotImplementedError("MTDistGenMove(rj=True) is the nested reversible-jump form: eryn_amd.rj.MTDistGenMoveRJ, a move of "
                                      "RJEnsembleSampler(rj_moves=...) on leaf-packing records")
        if symmetric:
            raise NotImplementedError("MTDistGenMove(symmetric=True) is not built: the device forms the weights of an independence "
                                      "proposal, logP - logq")
        if not independent:
            raise NotImplementedError("MTDistGenMove needs independent=True: the reference's default, independent=False, raises "
                                      "UnboundLocalError inside get_mt_proposal (multipletry.py:456), and the device builds the "
                                      "independent form only")
        if isinstance(num_try, bool) or not isinstance(num_try, numbers.Integral):
            raise ValueError("num_try must be an int")
        if not 1 <= int(num_try) <= MAX_TRY:
            raise ValueError(f"num_try must be in 1 .. {MAX_TRY} (one tile row per try)")
        self.num_try = int(num_try)
        self.independent, self.symmetric, self.rj = True, False, False
        if isinstance(generate_dist, dict) and generate_dist and all(isinstance(k, str) for k in generate_dist):
            containers = dict(generate_dist)
        else:
            containers = {None: generate_dist}             # (a bare container: the sampler's one branch)
        for key, dist in containers.items():
            if isinstance(dist, dict):
                dist = ProbDistContainer(dist)
            elif not isinstance(dist, ProbDistContainer) and not all(hasattr(dist, a) for a in ("priors_in", "rvs", "logpdf")):
                raise ValueError("Distributions need to be eryn.prior.ProbDistContainer object.")
            containers[key] = dist
        if len(containers) != 1:
            raise NotImplementedError("the device path handles a single branch")
        (self.branch_name, self.container), = containers.items()
        self.generate_dist = self.container
        # the terms the device reads: the container itself, or a foreign container through the dict it was made of
        self.spec = prior_spec(self.container if isinstance(self.container, ProbDistContainer) else dict(self.container.priors_in))
        self.log_sum_weights = self.aux_log_sum_weights = None
        MHMove.__init__(self, **kwargs)

    def device_proposal(self):
        """("mt_dist", prior_terms dict, num_try) for the context's MH slot (``HipEnsemble.set_mt_dist_proposal``)."""
        return "mt_dist", self.spec.terms, self.num_try

    def propose(self, model, state):
        name, br, T, W, D = self._single_branch(state)
        if self.spec.lo.shape != (D,):
            raise ValueError(f"generate_dist describes {self.spec.lo.shape[0]} parameters, the state has {D}")
        eng = self._ensure_engine(T, W, D)
        if hasattr(eng.likelihood, "evaluate"):
            raise NotImplementedError("MH moves on the device need a device likelihood")
        if self.rng == "philox":                                       # device-side draws (k_mt_dist)
            return self._propose_philox(model, state, mh_proposal=self.device_proposal())
        self._upload_if_needed(eng, state, br)
        want = ("mh",) + mh_slot_key(self.device_proposal())
        if getattr(eng, "_move_cfg", None) != want:                    # (the slot may hold another move of the mix)
            eng.set_mt_dist_proposal(self.spec.terms, self.num_try, 1.0)
            eng._move_cfg = want
        self._bump(eng)
        K = self.num_try
        q = np.asarray(self.container.rvs(size=(T * W, K)), dtype=np.float64).reshape(T, W, K, D)   # mtdistgen.py:70
        u_pick = np.random.rand(T * W)                                 # multipletry.py:57 (the global stream)
        u_acc = model.random.rand(T, W)                                # mh.py:157
        out = eng.mt_dist_step(q, u_pick, u_acc, want=("lsw", "aux_lsw"))
        accepted = out["keep"]
        self.log_sum_weights = out["lsw"].reshape(-1)                  # multipletry.py:490-491
        self.aux_log_sum_weights = out["aux_lsw"].reshape(-1)
        if self._accepted is not None:
            self.accepted += accepted                                  # mh.py:186
        self.num_proposals += 1
        return self._finish(eng, state, name, br, T, W), accepted
