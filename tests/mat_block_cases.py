"""What tests/test_mat_block_abi.py, tests/test_gpu_mat_mult_block.py and tests/test_gpu_mat_eigen.py share: the chunk plan of IGXMatMultBlock
restated in Python, and the oracle's Poisson and Mass matrices of the two vibration benchmarks the matrix-free eigen solve
refuses -- the membrane (dim 2, p = 3, 6^2 elements, all four faces Dirichlet) and the rod (dim 1, p = 2, 12 elements, both ends fixed)."""
import functools

import numpy as np

ACTION_BLOCK_MAX = 48
LOWDIM = {"membrane": dict(dim=2, p=3, N=(6, 6), nev=4, block=6), "rod": dict(dim=1, p=2, N=(12,), nev=2, block=3)}


def full_width(bs):
    """NC: the columns of a full chunk, 2 bs NC <= 32 accumulator registers"""
    return 8 if bs <= 2 else 4 if bs <= 4 else 2


def plan(bs, nx):
    """the widths of the launches for nx columns, in order: full chunks, then the next narrower widths, then a single column (Mat.mult's kernel)"""
    out, w = [], full_width(bs)
    while nx > 0:
        while w > nx:
            w //= 2
        out.append(w)
        nx -= w
    return out


@functools.lru_cache(maxsize=None)
def lowdim_oracle(name):
    """(A, B, free mask, nodes per axis) of the oracle: Poisson and Mass, every face Dirichlet"""
    from common import make_pair
    c = LOWDIM[name]
    mats, nodes = [], None
    for form in ("orc_form_poisson", "orc_form_mass"):
        orc, _ = make_pair(c["dim"], 1, c["p"], list(c["N"]), engine=False)
        for d in range(c["dim"]):
            for s in range(2):
                orc.set_boundary_value(d, s, 0, 0.0)
        Mx, _ = orc.compute_system(form)
        mats.append(Mx.scipy().tocsr())
        nodes = [orc.axis(i)["nnp"] for i in range(c["dim"])]
    edge = [np.isin(np.arange(n), (0, n - 1)) for n in nodes]
    fixed = edge[0] if c["dim"] == 1 else (edge[1][:, None] | edge[0][None, :]).reshape(-1)      # node r0 + n0 r1
    assert fixed.size == mats[0].shape[0]
    return mats[0], mats[1], ~fixed, nodes
