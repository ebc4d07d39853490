"""The plain-Python restatement of the exact transposition (tests/transpose_ref.py) against two hand-worked vectors at
tspace 4: it is the expected value of tests/test_parity_transpose_gpu.py, these literals are what it rests on."""
import transpose_ref as tr


def test_forward_vector():
    # source trace [(0, 2), (3, 4), (1, 4)] on A's grid
    ab, ae, bb, be, ops, tiles, follows = tr.transpose_record(2, 11, 3, 13, 0, [0, 0, 3, 1, 0, 2, 0, 0, 2, 0, 0], 4)
    assert (ab, ae, bb, be) == (3, 13, 2, 11)
    assert ops.tolist() == [0, 0, 3, 2, 0, 1, 0, 0, 1, 0, 0]
    assert tiles == [(0, 1), (3, 4), (1, 3), (0, 1)]
    assert sum(d for d, _ in tiles) == 4 and follows == 0


def test_comp_vector():
    # source trace [(1, 3), (1, 3)]; the code-2 op right after grid point 8 lies in the second tile
    ab, ae, bb, be, ops, tiles, follows = tr.transpose_record(5, 12, 1, 7, 1, [0, 3, 0, 1, 0, 0, 0], 4, alen=20, blen=12)
    assert (ab, ae, bb, be) == (5, 11, 8, 15)
    assert ops.tolist() == [0, 0, 0, 2, 0, 3, 0]
    assert tiles == [(0, 3), (2, 4)] and follows == 1
    # the same ops without the reversal (a forward record over the same A' interval) give another trace
    _, _, _, _, _, unreversed, _ = tr.transpose_record(8, 15, 5, 11, 0, [0, 3, 0, 1, 0, 0, 0], 4)
    assert unreversed == [(1, 3), (1, 4)]


def test_end_points_on_the_grid_and_a_single_tile():
    # abpos' and aepos' on the grid: neither is a grid point of the record, one tile between them and the next point
    _, _, _, _, _, tiles, _ = tr.transpose_record(0, 8, 4, 12, 0, [0] * 8, 4)
    assert tiles == [(0, 4), (0, 4)]
    _, _, _, _, _, tiles, _ = tr.transpose_record(1, 4, 5, 8, 0, [0, 3, 0], 4)
    assert tiles == [(1, 3)]
