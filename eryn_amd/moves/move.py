"""Move base with the attributes EnsembleSampler relies on (eryn/moves/move.py:68-221, 404-457)."""
import numpy as np


class Move:
    def __init__(self, temperature_control=None, periodic=None, gibbs_sampling_setup=None,
                 prevent_swaps=False, skip_supp_names_update=[], is_rj=False, use_gpu=None,
                 random_seed=None, **kwargs):
        self._initialize_branch_setup(gibbs_sampling_setup, is_rj=is_rj)
        self.periodic = periodic
        self.prevent_swaps = prevent_swaps
        self.is_rj = is_rj
        self.num_proposals = 0
        self.time = 0
        self._accepted = None
        if random_seed is not None:          # move.py:94-96: seeds the *global* stream
            np.random.seed(random_seed)
        self.temperature_control = temperature_control

    # -- Gibbs parameter blocks (move.py:113-221) ---------------------------------------------------------
    def _initialize_branch_setup(self, gibbs_sampling_setup, is_rj=False):
        """``gibbs_sampling_setup`` in the reference's forms - a branch name (every parameter), ``(name, mask)`` with ``mask`` None
        or a 2-D bool array ``(nleaves_max, ndim)``, a dict ``{name: mask | None}`` (one block), or a list of those - into
        ``self.gibbs_sampling_setup``: None, or one entry per block, each a list of ``(name, mask | None)``.  The reference's
        ``ValueError``s for everything else, and one of this package's own for an empty list."""
        self.gibbs_sampling_setup_input = gibbs_sampling_setup
        self.gibbs_sampling_setup = None
        if gibbs_sampling_setup is None:
            return
        if type(gibbs_sampling_setup) not in (str, tuple, list, dict):
            raise ValueError("gibbs_sampling_setup must be string, dict, tuple, or list.")
        items = gibbs_sampling_setup if isinstance(gibbs_sampling_setup, list) else [gibbs_sampling_setup]
        if not items:          # (the reference takes an empty list and then proposes nothing, ever: no device context steps "no move")
            raise ValueError("gibbs_sampling_setup is an empty list: a move needs at least one block to propose")

        def checked(mask):
            if mask is not None and is_rj:
                raise ValueError("inputting gibbs indexing at the leaf/parameter level is not allowed with an RJ proposal. Only branch names.")
            if (mask is not None and not isinstance(mask, np.ndarray)) or (isinstance(mask, np.ndarray) and mask.ndim != 2):
                raise ValueError("When inputing gibbs indexing and using a 2-tuple, second item must be None or 2D np.ndarray of shape (nleaves_max, ndim).")
            return mask

        blocks = []
        for item in items:
            if isinstance(item, str):
                blocks.append([(item, None)])
            elif isinstance(item, tuple):
                assert len(item) == 2
                blocks.append([(item[0], checked(item[1]))])
            elif isinstance(item, dict):
                blocks.append([(key, checked(value)) for key, value in item.items()])
            else:
                raise ValueError("If providing a list for gibbs_sampling_setup, each item needs to be a string, tuple, or dict.")
        self.gibbs_sampling_setup = blocks

    def gibbs_masks(self, name, ndim):
        """The blocks as a bool array ``[nblocks, ndim]`` for the single branch ``name`` with ``nleaves_max == 1`` (None without a
        setup): a branch name alone is every parameter, a mask must be ``(1, ndim)``."""
        if self.gibbs_sampling_setup is None:
            return None
        out = []
        for block in self.gibbs_sampling_setup:
            if len(block) != 1 or block[0][0] != name:
                raise ValueError(f"gibbs_sampling_setup names {[b[0] for b in block]}: this move steps the single branch '{name}'")
            mask = block[0][1]
            if mask is None:
                out.append(np.ones(ndim, dtype=bool))
                continue
            if mask.shape != (1, ndim):
                raise ValueError(f"a gibbs_sampling_setup mask must have shape (nleaves_max, ndim) = (1, {ndim}), not {mask.shape}")
            out.append(mask[0].astype(bool))
        return np.stack(out)

    # -- periodic parameters (move.py:24-26,82): a PeriodicContainer (this package's or the reference's) or None.  The
    #    reference's sampler also assigns this attribute after construction when it was given one (ensemble.py:528-536).
    #    The device moves hand the periods to their context before every proposal (DeviceMove._apply_periodic).
    @property
    def periodic(self):
        return self._periodic

    @periodic.setter
    def periodic(self, periodic):
        if periodic is not None and not isinstance(periodic, dict) and not (
                hasattr(periodic, "inds_periodic") and hasattr(periodic, "periods")):
            raise ValueError("periodic must be PeriodicContainer or dict if not None.")
        self._periodic = periodic

    # -- counters (move.py:404-421) --------------------------------------------------------------
    @property
    def accepted(self):
        if self._accepted is None:
            raise ValueError("accepted must be inititalized with the init_accepted function if you want to use it.")
        return self._accepted

    @accepted.setter
    def accepted(self, accepted):
        assert isinstance(accepted, np.ndarray)
        self._accepted = accepted

    @property
    def acceptance_fraction(self):
        return self.accepted / self.num_proposals

    # -- tempering wiring (move.py:428-441) --------------------------------------------------------
    @property
    def temperature_control(self):
        return self._temperature_control

    @temperature_control.setter
    def temperature_control(self, temperature_control):
        self._temperature_control = temperature_control
        self.ntemps = 1 if temperature_control is None else temperature_control.ntemps

    def compute_log_posterior_basic(self, logl, logp):
        return logl + logp

    def tune(self, state, accepted):
        """Place holder for tuning, called by the sampler after every proposal when ``tune=True`` (move.py:459-470,
        ensemble.py:983-984)."""
        pass

    def propose(self, model, state):
        raise NotImplementedError("The proposal must be implemented by subclasses")
