"""Where the p = 3 rows walk stages an entry (rows3_stage_offset, petiga_amd/csrc/gram_rows3.hpp) through the host side the library
exposes (IGXRows3StageOffset), without a GPU.  On a full layer of a regular tile the run (column, dy, dx) of patch_run_address has
RB = 7 x 7, RC = P2 c1 + P1 with c1 = 7 and band positions P2 = dy + 3, P1 = dx + 3 on axes 2 and 1, and the layer table has
P0[d] = d + 3: the entry lies RC 7 + P0[d] doubles into its column's row, and the buffer holds the nine rows of 343 one after the other."""
import numpy as np

import petiga_amd as P

COLS, BW, ROW = 9, 7, 343


def test_offset_is_the_entry_s_place_in_its_row():
    seen = []
    for col in range(COLS):
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                rc = (dy + 3) * BW + (dx + 3)
                for d in range(-3, 4):
                    off, n = P.rows3_stage_offset(col, dy, dx, d)
                    assert n == COLS * ROW
                    assert off == col * ROW + rc * BW + (d + 3)
                    seen.append(off)
    # every double of the buffer is one entry's: the copy to memory moves whole rows
    assert np.array_equal(np.sort(seen), np.arange(COLS * ROW))


def test_a_run_is_seven_consecutive_doubles():
    for col in (0, 4, 8):
        for dy, dx in ((-3, -3), (0, 0), (3, 3), (-1, 2)):
            offs = [P.rows3_stage_offset(col, dy, dx, d)[0] for d in range(-3, 4)]
            assert offs == list(range(offs[0], offs[0] + BW))
