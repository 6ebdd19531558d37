"""Host-side bounds check of the early-stop plans (CPU, no GPU): ldpc_debug_bs_bounds with flags
bit 2 (LDPC_BOUNDS_ES) also plans the ES instances of kBsInst -- their syndrome words in the RED
region, and the hard-decision / syndrome reads that those builds make at every iteration whether
or not UCN weights are set -- and every read must stay inside its allocation.  Without the bit the
function checks, and counts, exactly the plans it did before the mode existed."""
import pytest

from test_bs_bounds import bounds, lib  # noqa: F401  (the module's library fixture)

ES = 4
WMAN, WIFI = ("wman_N0576_R34_z24", 24), ("802_11n_N648_R56_z27", 27)
BG1 = ("5G_LDPC_R0.73_n_dec2304_n2112_k1536_z72_s1537_1584", 72)
BG2 = ("5G_LDPC_R0.50_n_dec1280_n1024_k512_z64_s513_640", 64)

# plans checked without the bit, recorded from the commit before the mode: (graph, au, bu) -> count
# (the same at T = 1, 20 and 50)
BEFORE = {(WMAN, 1, 1): 5, (WMAN, 0, 0): 4, (WIFI, 1, 1): 2, (WIFI, 0, 0): 0,
          (BG1, 1, 1): 2, (BG1, 0, 0): 0, (BG2, 1, 1): 7, (BG2, 0, 0): 6}


@pytest.mark.parametrize("name,z", [WMAN, WIFI])
@pytest.mark.parametrize("T", [1, 20, 50])
@pytest.mark.parametrize("au,bu", [(1, 1), (0, 0), (0, 1), (1, 0)])
def test_es_plans_read_inside_their_allocations(lib, name, z, T, au, bu):  # noqa: F811
    n0, v0, _ = bounds(lib, name, z, T, au=au, bu=bu)
    n, v, msg = bounds(lib, name, z, T, au=au, bu=bu, flags=ES)
    assert v == 0, msg
    # the ES instance's plans (with and without UCN weights) on top of the others
    assert n >= 1 and n == n0 + 2, (n0, n)


@pytest.mark.parametrize("q", [5, -5, 4, 3])
def test_es_plans_on_every_grid(lib, q):  # noqa: F811
    for name, z in (WMAN, WIFI):
        n0, _, _ = bounds(lib, name, z, 20, q=q)
        n, v, msg = bounds(lib, name, z, 20, q=q, flags=ES)
        assert n == n0 + 2 and v == 0, (name, q, n0, n, msg)


@pytest.mark.parametrize("T", [1, 20, 50])
def test_count_without_the_bit_is_the_parents(lib, T):  # noqa: F811
    for ((name, z), au, bu), want in BEFORE.items():
        n, v, msg = bounds(lib, name, z, T, au=au, bu=bu)
        assert (n, v) == (want, 0), (name, au, bu, n, msg)


def test_multi_chunk_graphs_have_no_es_plan(lib):  # noqa: F811
    for name, z in (BG1, BG2):
        assert bounds(lib, name, z, 20, flags=ES)[0] == bounds(lib, name, z, 20)[0]
