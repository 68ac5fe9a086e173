"""The p = 3 patch walk's ticket -> item map (patch3_ticket_item, petiga_amd/csrc/gram_patch3.hpp) through the host side the library
exposes (IGXPatch3TicketOrder), without a GPU: a permutation of the colour's items in both orders, for the meshes of
tests/test_gpu_patch3_tickets.py in every colour and for the 5504 items of colour (1, 0) at 256^3 in four segments; and with the faces
first, no interior patch ahead of a face patch of the same segment."""
import numpy as np
import pytest

import petiga_amd as P

MX, MY, SX, SY = 4, 2, 2, 3      # the patch of pencils and the colours per axis (PATCH3_MX, PATCH3_MY; Patch3::SX, SY)
# (n1, n2) of the GPU cases, with the segment counts they can be walked in; 256^3
MESHES = [((9, 7), (5,)), ((4, 2), (1, 2, 4)), ((5, 4), (3,)), ((3, 3), (1, 2, 4)), ((256, 256), (4,))]
CASES = [(n, nseg, cx, cy) for n, segs in MESHES for nseg in segs for cy in range(SY) for cx in range(SX)]


def _count(n, nseg, cx, cy):
    npx, npy = -(-n[0] // MX), -(-n[1] // MY)
    return max(0, -(-(npx - cx) // SX)) * max(0, -(-(npy - cy) // SY)) * nseg


def test_headline_colour_has_5504_items():
    assert _count((256, 256), 4, 1, 0) == 5504
    assert len(P.patch3_ticket_order(256, 256, 4, 1, 0)[0]) == 5504


@pytest.mark.parametrize("n,nseg,cx,cy", CASES)
@pytest.mark.parametrize("order", [0, 1])
def test_tickets_are_a_permutation_of_the_items(n, nseg, cx, cy, order):
    items, faces = P.patch3_ticket_order(n[0], n[1], nseg, cx, cy, order)
    assert len(items) == _count(n, nseg, cx, cy)
    assert np.array_equal(np.sort(items), np.arange(len(items)))
    if order == 0:
        assert np.array_equal(items, np.arange(len(items)))
    # a patch is on a face or not whatever the order and the segment
    if len(items):
        patches = len(items) // nseg
        nat = P.patch3_ticket_order(n[0], n[1], nseg, cx, cy, 0)[1]
        assert np.array_equal(faces, nat[items])
        assert all(np.array_equal(nat[:patches], nat[s * patches:(s + 1) * patches]) for s in range(nseg))
        # ... and it is the patch's place in the mesh that says so
        npx, npy = -(-n[0] // MX), -(-n[1] // MY)
        pxc = -(-(npx - cx) // SX)
        ppx, ppy = cx + (np.arange(patches) % pxc) * SX, cy + (np.arange(patches) // pxc) * SY
        assert np.array_equal(nat[:patches] != 0, (ppx == 0) | (ppx == npx - 1) | (ppy == 0) | (ppy == npy - 1))


@pytest.mark.parametrize("n,nseg,cx,cy", CASES)
def test_faces_first(n, nseg, cx, cy):
    items, faces = P.patch3_ticket_order(n[0], n[1], nseg, cx, cy, 1)
    if not len(items):
        return
    seg = items // (len(items) // nseg)
    for s in range(nseg):
        f = faces[seg == s]
        assert not np.any(np.diff(f) > 0)      # no interior patch comes before a face patch of the same segment
