"""Reading the fixtures under tests/golden/.

A fixture is NAME.npz.  One whose arrays hold more than SPLIT_ABOVE bytes is written in pieces of at most PART_BYTES (its
arrays in the order the generator recorded them): NAME.npz with the first ones, then NAME.part1.npz, NAME.part2.npz, ...
(tests/golden/make_golden.py, save), so that no committed file exceeds 1 MiB.  ``load`` joins the pieces."""
import glob
import os

import numpy as np

SPLIT_ABOVE = 1 << 20          # (the same figures as tests/golden/make_golden.py)
PART_BYTES = 1 << 19


class Fixture(dict):
    """The arrays of one fixture: ``fx[key]`` and ``fx.files``, as np.load's NpzFile offers them."""

    @property
    def files(self):
        return list(self)


def load(golden_dir, name):
    fx = Fixture()
    parts = sorted(glob.glob(os.path.join(golden_dir, glob.escape(name) + ".part*.npz")),
                   key=lambda p: int(p.rsplit(".part", 1)[1][:-len(".npz")]))
    for p in [os.path.join(golden_dir, name + ".npz")] + parts:
        with np.load(p) as f:
            fx.update((k, f[k]) for k in f.files)
    return fx
