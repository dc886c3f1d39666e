"""The CPU half of tests/test_gpu_wide_positions.py where no GPU exists: expected(name) builds every value the device legs compare against from the oracle and
the models alone, and each leg's value function asserts on the way that its inputs reach the edges and hold the kinds of walk and line the leg is for.  Built
here for A (4-byte positions, the sign bit and the values below the sentinel) and C (2^38): B shares A's construction."""
import pytest

from test_gpu_wide_positions import EDGES, SAM_KS, WALK_KS, expected


@pytest.mark.parametrize("name", ["A", "C"])
def test_expected_values_reach_their_edges(name):
    E = expected(name)
    try:
        assert E.n > EDGES[name][-1]
        assert set(E.left["want"]) == set(E.right["want"]) == set(WALK_KS) and len(E.left["row"]) > 300 and len(E.right["row"]) > 300
        assert len(E.x_sam) == 3 * 2 * 2 * 2 * len(SAM_KS) and len(E.x_reads) == len(E.sam_reads) + 150
    finally:
        E.o.close()
        E.ot.close()
        expected.cache_clear()
