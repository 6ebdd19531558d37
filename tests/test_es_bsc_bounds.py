"""Host-side bounds check of the compressed kernel's early-stop plan (CPU, no GPU):
ldpc_debug_bs_bounds with flags bit 3 (LDPC_BOUNDS_ES_BSC) also plans the early-stop build of bsc
where a decode in the mode would take it -- no bsl plan serves the graph and every channel weight
is 1: 5G BG1 -- and checks its T syndrome words (inside the RED region, before the alpha table),
its LDS size and the bsc plan's own chunk / position / channel-table checks.  It counts as one
more plan; without the bit the counts are what they were (tests/test_es_bounds.py pins them)."""
import pytest

from test_bs_bounds import BIG_TABLES, bounds, lib  # noqa: F401  (the module's library fixture)

ES, ES_BSC = 4, 8
WMAN, WIFI = ("wman_N0576_R34_z24", 24), ("802_11n_N648_R56_z27", 27)
BG1 = ("5G_LDPC_R0.73_n_dec2304_n2112_k1536_z72_s1537_1584", 72)
BG2 = ("5G_LDPC_R0.50_n_dec1280_n1024_k512_z64_s513_640", 64)


@pytest.mark.parametrize("T", [1, 20, 50])
@pytest.mark.parametrize("au", [1, 0])
def test_bg1_es_plan_reads_inside_its_allocations(lib, T, au):  # noqa: F811
    n0, v0, msg0 = bounds(lib, *BG1, T, au=au, bu=1)
    n, v, msg = bounds(lib, *BG1, T, au=au, bu=1, flags=ES_BSC)
    assert v0 == 0, msg0
    assert v == 0, msg
    assert n0 >= 1 and n == n0 + 1, (n0, n)


@pytest.mark.parametrize("q", [5, -5, 4, 3])
def test_bg1_es_plan_on_every_grid(lib, q):  # noqa: F811
    n0, _, _ = bounds(lib, *BG1, 20, q=q)
    n, v, msg = bounds(lib, *BG1, 20, q=q, flags=ES_BSC)
    assert n == n0 + 1 and v == 0, (q, n0, n, msg)


@pytest.mark.parametrize("name,z", [WMAN, WIFI, BG2])
@pytest.mark.parametrize("au,bu", [(1, 1), (0, 1), (0, 0), (1, 0)])
def test_graphs_that_bsl_serves_have_no_bsc_es_plan(lib, name, z, au, bu):  # noqa: F811
    for T in (1, 20, 50):
        assert bounds(lib, name, z, T, au=au, bu=bu, flags=ES_BSC) == bounds(lib, name, z, T, au=au, bu=bu)
        # (and the bit leaves the bsl early-stop plans' count alone)
        assert bounds(lib, name, z, T, au=au, bu=bu, flags=ES | ES_BSC) == bounds(lib, name, z, T, au=au, bu=bu, flags=ES)


@pytest.mark.parametrize("au", [1, 0])
def test_bg1_without_beta_one_has_no_es_plan(lib, au):  # noqa: F811
    """Per-column channel weights (beta not all ones): the early-stop build rests on the beta = 1
    identity Tv sign = APP sign, so there is no plan to check."""
    for T in (1, 20, 50):
        assert bounds(lib, *BG1, T, au=au, bu=0, flags=ES_BSC) == bounds(lib, *BG1, T, au=au, bu=0)


def test_oversized_channel_tables_are_caught_on_the_es_plan(lib):  # noqa: F811
    """The Q8 early-stop build borrows the SGN region for the sampler's tables as the full-T build
    does: told that they are 4 bytes longer than that region, the early-stop plan reports it too."""
    n0, v0, _ = bounds(lib, *BG1, 50, flags=BIG_TABLES)
    n, v, msg = bounds(lib, *BG1, 50, flags=ES_BSC | BIG_TABLES)
    assert n == n0 + 1 and v0 > 0 and v > v0 and "channel tables" in msg, (n0, n, v0, v, msg)
