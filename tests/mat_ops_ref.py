"""numpy restatement of the table-driven column rule of the stored matrix (petiga_amd/csrc/mat_ops.hpp, k_browptr / k_bcolidx in engine.hip),
written from the layout's statement: row r = (r0, r1, r2) owns c0 c1 c2 blocks, c_d = rcnt[d][r_d]; block k = k0 + c0 (k1 + c1 k2) has the
column node rcol[0][r0][k0] + ncol0 (rcol[1][r1][k1] + ncol1 rcol[2][r2][k2]).  From the per-axis tables alone it rebuilds browptr and bcolidx
and finds the position of every row's diagonal block; entrywise_product() is the long double product the GPU tests hold IGXMatMult to."""
import numpy as np


def axis_tables(stencils, width=None):
    """(rcnt [nrow], rcol [nrow][width]) of one axis from each row's stencil, a list of column indices that may repeat (a periodic axis with
    fewer than 2p+1 functions wraps onto itself): the distinct columns ascending, padded with -1 -- AxisLayout::rcnt / rcol of host.cpp"""
    rows = [sorted(set(int(c) for c in s)) for s in stencils]
    width = max(len(r) for r in rows) if width is None else width
    rcnt = np.array([len(r) for r in rows], dtype=np.int64)
    rcol = np.full((len(rows), width), -1, dtype=np.int64)
    for i, r in enumerate(rows):
        rcol[i, :len(r)] = r
    return rcnt, rcol


def unit_axis():
    """an axis beyond dim: one row, one column"""
    return np.array([1], dtype=np.int64), np.array([[0]], dtype=np.int64)


def _rows(rcnt):
    n0, n1, n2 = (len(c) for c in rcnt)
    r = np.arange(n0 * n1 * n2, dtype=np.int64)
    return r % n0, (r // n0) % n1, r // (n0 * n1)


def browptr(rcnt):
    """[nbrows + 1]: the first block of every row, rows ordered r0 + nrow0 (r1 + nrow1 r2)"""
    r0, r1, r2 = _rows(rcnt)
    return np.concatenate([[0], np.cumsum(rcnt[0][r0] * rcnt[1][r1] * rcnt[2][r2])]).astype(np.int64)


def bcolidx(rcnt, rcol, ncol):
    """the column node of every block, in storage order"""
    r0, r1, r2 = _rows(rcnt)
    c0, c1 = rcnt[0][r0], rcnt[1][r1]
    rp = browptr(rcnt)
    row = np.repeat(np.arange(r0.size), np.diff(rp))
    k = np.arange(rp[-1], dtype=np.int64) - rp[row]
    k0, k1, k2 = k % c0[row], (k // c0[row]) % c1[row], k // (c0[row] * c1[row])
    col = rcol[0][r0[row], k0] + ncol[0] * (rcol[1][r1[row], k1] + ncol[1] * rcol[2][r2[row], k2])
    assert (col >= 0).all()
    return col.astype(np.int64)


def diagonal_position(rcnt, rcol):
    """[nbrows]: k of the block whose column node is the row's own node (one rank: column index = row index on every axis), -1 where a row
    does not hold it"""
    r0, r1, r2 = _rows(rcnt)
    pos = []
    for d, rd in enumerate((r0, r1, r2)):
        hit = rcol[d] == np.arange(len(rcnt[d]))[:, None]
        at = np.where(hit.any(axis=1), hit.argmax(axis=1), -1)
        pos.append(at[rd])
    k = pos[0] + rcnt[0][r0] * (pos[1] + rcnt[1][r1] * pos[2])
    return np.where((pos[0] >= 0) & (pos[1] >= 0) & (pos[2] >= 0), k, -1)


def tables_of_pattern(rp, ci, nrow, ncol):
    """the per-axis tables back out of a block pattern (browptr, bcolidx) of a tensor-product matrix: axis d's stencil of row r_d is read from
    the row with the other two indices 0.  What the GPU tests feed the restatement with, so that it is checked against the engine's own pattern."""
    rcnt, rcol = [], []
    stride = (1, ncol[0], ncol[0] * ncol[1])
    rstride = (1, nrow[0], nrow[0] * nrow[1])
    for d in range(3):
        st = []
        for r in range(nrow[d]):
            row = r * rstride[d]
            cols = np.asarray(ci[rp[row]:rp[row + 1]], dtype=np.int64)
            st.append(sorted(set(((cols // stride[d]) % ncol[d]).tolist())))
        c, t = axis_tables(st)
        rcnt.append(c)
        rcol.append(t)
    return rcnt, rcol


def entrywise_product(rp, ci, val, bs, x):
    """(y, S, n) per scalar row in np.longdouble: y = A x, S = sum_j |a_rj| |x_j| and n = the number of products of the row"""
    nb = len(rp) - 1
    blocks = np.asarray(val, dtype=np.longdouble).reshape(-1, bs, bs)
    xb = np.asarray(x, dtype=np.longdouble).reshape(-1, bs)[np.asarray(ci, dtype=np.int64)]          # [nblocks][bs]
    prod = np.einsum("kij,kj->ki", blocks, xb)
    mag = np.einsum("kij,kj->ki", np.abs(blocks), np.abs(xb))
    row = np.repeat(np.arange(nb), np.diff(rp))
    y, S = np.zeros((nb, bs), dtype=np.longdouble), np.zeros((nb, bs), dtype=np.longdouble)
    np.add.at(y, row, prod)
    np.add.at(S, row, mag)
    n = np.repeat(np.diff(rp) * bs, bs)
    return y.reshape(-1), S.reshape(-1), n
