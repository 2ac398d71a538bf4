"""CPU: the index arithmetic of the ring form of the direct searches (csrc/me_kernel.hip: run_ring_searches, ring_rows), restated in
Python.  A lane is (request, slice of the block rows); a lane walks the window rows under its slice once and adds window row j to every
search row y with (j - y) a multiple of rs.  For every nreq 1..64, sa_h 1..3, rs 1..2 and 1..64 compared rows: each (request, search row,
block row) triple is covered exactly once, by the window row the search reads there, and no packed accumulator takes more rows between two
flushes than its 16-bit lanes hold."""
import pytest

THREADS = 64


def ring_geometry(nreq, rows):
    """(lg, S, rows_per): G = 1 << lg lanes per request, S of them at work on rows_per block rows each (the last one on the rest)"""
    lg = 0
    while (2 << lg) * nreq <= THREADS:
        lg += 1
    s0 = min(rows, 1 << lg)
    rows_per = (rows + s0 - 1) // s0
    return lg, (rows + rows_per - 1) // rows_per, rows_per


def lane_of(req, sl, lg):
    return (req << lg) + sl


def slice_pairs(sl, rows, rows_per, rs, sa_h, rows_per_flush):
    """What the lane of slice `sl` does: [(window row relative to the request's row 0, search row y, block row)], its step count, and the
    longest run of rows any accumulator takes without a flush"""
    e0 = sl * rows_per
    mine = min(e0 + rows_per, rows) - e0
    steps_max = rs * (rows_per - 1) + sa_h  # uniform loop bound
    steps = rs * (mine - 1) + sa_h          # rows this lane's pieces are fetched for
    out, held, worst = [], [0] * sa_h, 0
    for j in range(steps_max):
        for y in range(sa_h):
            dd = j - y
            if dd < 0 or dd % rs:
                continue
            t = dd // rs
            if t >= rows_per:
                continue
            if t < mine:
                assert j < steps, "a row that was not fetched"
                out.append((e0 * rs + j, y, e0 + t))
                held[y] += 1
                worst = max(worst, held[y])
            if (t + 1) % rows_per_flush == 0 or t + 1 == rows_per:
                held[y] = 0
    assert held == [0] * sa_h, "sums left in a packed accumulator"
    return out, steps, worst


@pytest.mark.parametrize("nreq", range(1, 65))
def test_lanes_are_distinct_and_a_requests_slices_are_neighbours(nreq):
    for rows in range(1, 65):
        lg, S, rows_per = ring_geometry(nreq, rows)
        G = 1 << lg
        assert G * nreq <= THREADS and (2 * G * nreq > THREADS or G == THREADS)
        assert 1 <= S <= min(rows, G) and (S - 1) * rows_per < rows <= S * rows_per
        lanes = [lane_of(r, s, lg) for r in range(nreq) for s in range(S)]
        assert len(set(lanes)) == len(lanes) and max(lanes) < THREADS
        for r in range(nreq):  # one aligned group of G lanes: what the DPP sum runs over
            assert {lane_of(r, s, lg) >> lg for s in range(S)} == {r}
            assert [lane_of(r, s, lg) & (G - 1) for s in range(S)] == list(range(S))


@pytest.mark.parametrize("rs", (1, 2))
@pytest.mark.parametrize("sa_h", (1, 2, 3))
@pytest.mark.parametrize("ndw", (8, 16), ids=["32-wide", "64-wide"])
def test_every_triple_is_covered_once(ndw, sa_h, rs):
    rows_per_flush = 64 // ndw
    seen_geometry = set()
    for nreq in range(1, 65):
        for rows in range(1, 65):
            lg, S, rows_per = ring_geometry(nreq, rows)
            if (S, rows_per, rows) in seen_geometry:  # the requests are alike: a request's cover depends on its slices only
                continue
            seen_geometry.add((S, rows_per, rows))
            cover = {}
            for sl in range(S):
                pairs, steps, worst = slice_pairs(sl, rows, rows_per, rs, sa_h, rows_per_flush)
                assert worst <= rows_per_flush
                assert steps == rs * (min((sl + 1) * rows_per, rows) - sl * rows_per - 1) + sa_h
                for wrow, y, row in pairs:
                    assert wrow == y + rs * row  # search row y at block row `row` reads this window row
                    assert (y, row) not in cover
                    cover[(y, row)] = sl
            assert set(cover) == {(y, row) for y in range(sa_h) for row in range(rows)}
