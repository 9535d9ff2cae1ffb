"""K2, K3 and K4 alone at the shapes where they change code path: constructed segments on both sides of every limit written
into k34_segments.hip (short-path width and tile halo, 512 leaders on chip, 1 024 edges in LDS, the u16 count that wraps), and the
radix sort on skewed keys, payloads with a non-zero high half, unaligned views, every tile count around the persistent grid
and a bit field that does not start at bit 0.  The checkers are the harness programs' own sequential restatements
(tests/harness/seg_kernels_test.hip, sort_bench.hip): greedy scan in insertion order with a real uint16_t count, stable sort + unique,
std::stable_sort on the sorted bit field."""
import os
import re
import subprocess

import pytest

import pagctl

BIN = os.path.join(pagctl.ROOT, "tests", "harness", "bin")
SEG = os.path.join(BIN, "seg_kernels_test")
SORT = os.path.join(BIN, "sort_bench")

# (seg_kernels_test list prints the same names; a name the program does not know fails its test)
SEG_CASES = [
    # short path: a segment of W - 1, W, W + 1 records (W = 32, 64) with its head at record 0, at the last owned record of a tile (the
    # body in the halo), at the first record of the next tile; ending with the stream at n = 1, OWN, OWN + 1, 512, 513; one segment
    # that is the whole stream.  Each at eps 0, 1, 10, 3 000, 2^30 and 2^31 + 5.
    "short_at_stream_start", "short_at_last_owned", "short_at_next_tile", "short_end_n1", "short_end_nOWN", "short_end_nOWN1",
    "short_end_n512", "short_end_n513", "short_whole_stream_200000",
    # the 512 leaders cluster_long keeps in registers; an item similar to two leaders joins the one inserted first
    "leaders_511", "leaders_512", "leaders_513", "leaders_513th_is_last_item", "leaders_1500", "first_leader_wins_on_chip",
    "first_leader_wins_on_chip_swapped", "first_leader_wins_in_place", "first_leader_wins_in_place_swapped",
    # the 1 024 edge records edges_long sorts in LDS
    "edges_1023", "edges_1024", "edges_1025", "edges_100000_of_64_groups",
    # clusters of 65 535, 65 536, 65 537 and 131 073 items: counts 65 535, 0, 1, 1
    "wrap_on_chip_pass1", "wrap_on_chip_pass2", "wrap_in_place_leader0_pass1", "wrap_in_place_leader0_pass2",
    "wrap_in_place_leader600_pass1", "wrap_in_place_leader600_pass2",
]

# Slowest case on an MI355X: short_whole_stream_200000, 14.3 s (wall time of the test, all its eps), then edges_100000_of_64_groups,
# 13.1 s: nearly all of it edges_long's rank sort of 100 000 records through memory; every other case takes less than a second.  The
# timeout is more than ten times that.
SEG_TIMEOUT = 300


def _describe(name, wide):
    r = subprocess.run([SEG, "describe", name, str(wide)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return [{k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", line)} for line in r.stdout.splitlines() if line.startswith("segment")]


@pytest.mark.parametrize("wide", [0, 1])
def test_constructed_cases_have_the_shapes_they_are_named_for(wide):
    """The condition on the INPUT of every constructed case, from the sequential scan alone (no device): heads at the tile offsets, leader
    counts, cluster sizes and edge counts on the very limits.  Keeps a change of the generators from moving a case off its limit."""
    assert os.path.exists(SEG), "run `make harness`"
    assert subprocess.run([SEG, "list"], capture_output=True, text=True).stdout.split() == SEG_CASES
    own = 448 if wide else 480
    lens = [31, 32, 33, 63, 64, 65]
    for name, head in (("short_at_stream_start", 0), ("short_at_last_owned", own - 1), ("short_at_next_tile", own)):
        segs = _describe(name, wide)
        assert [s["records"] for s in segs] == lens and all(s["head"] == head for s in segs), name
    assert [s["tile_offset"] for s in _describe("short_at_last_owned", wide)] == [own - 1] * 6
    for name, n in (("short_end_nOWN", own), ("short_end_nOWN1", own + 1), ("short_end_n512", 512), ("short_end_n513", 513)):
        segs = _describe(name, wide)
        assert [s["records"] for s in segs] == lens and all(s["ends_at_n"] == 1 and s["head"] + s["records"] == n for s in segs), name
    assert [(s["records"], s["ends_at_n"]) for s in _describe("short_end_n1", wide)] == [(1, 1)]
    assert [(s["records"], s["head"], s["ends_at_n"]) for s in _describe("short_whole_stream_200000", wide)] == [(200000, 0, 1), (100000, 0, 1)]
    for nl in (511, 512, 513, 1500):
        assert [s["leaders"] for s in _describe(f"leaders_{nl}", wide)] == [nl, nl]
    segs = _describe("leaders_513th_is_last_item", wide)
    assert [(s["leaders"], s["last_item_is_leader"]) for s in segs] == [(513, 1), (513, 1)]
    assert all(s["records"] > 3000 for s in segs)
    for name, nl in (("first_leader_wins_on_chip", 300), ("first_leader_wins_in_place", 700)):
        for suffix in ("", "_swapped"):
            assert [s["leaders"] for s in _describe(name + suffix, wide)] == [nl]
    for m in (1023, 1024, 1025):
        segs = _describe(f"edges_{m}", wide)
        assert [s["records"] for s in segs] == [m] and segs[0]["edge_groups"] < m // 2
    assert [(s["records"], s["edge_groups"]) for s in _describe("edges_100000_of_64_groups", wide)] == [(100000, 64)]
    for name in SEG_CASES:
        if name.startswith("wrap_"):
            segs = _describe(name, wide)
            assert [s["biggest_cluster"] for s in segs] == [65535, 65536, 65537, 131073], name
            assert [s["leaders"] for s in segs] == [40 if "on_chip" in name else 700] * 4, name


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("name", SEG_CASES)
def test_segment_kernels_constructed_case(name, wide):
    """One constructed case through launch_cluster and launch_edges, both widths of the short path: seg_len of every slot, values, counts,
    the three / two counters, the one-record neighbours and the guard words around every array.  The short-path cases run at six
    eps (the last two take the plain predicate: 2 * eps overflows in SimForm).  Slowest case on an MI355X: short_whole_stream_200000, 14.3 s (K3 on
    200 000 records at six eps, K4 on 100 000: K4's through-memory sort took 50 s for 200 000)."""
    assert os.path.exists(SEG), "run `make harness`"
    r = subprocess.run([SEG, "case", name, str(wide), "all"], capture_output=True, text=True, timeout=SEG_TIMEOUT)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and f"OK: case {name}" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("eps", [0, 1, 3000, 1 << 30, (1 << 31) + 5])
def test_segment_kernels_random_mode_at_eps(eps, wide):
    """The random segment lengths of test_segment_kernels_match_sequential_restatement (which runs at eps 10) at the other eps."""
    assert os.path.exists(SEG), "run `make harness`"
    r = subprocess.run([SEG, "20000", "2", str(wide), str(eps)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"eps {eps}" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("eps", [0, 3000, (1 << 31) + 5])
def test_segment_kernels_random_mode_over_the_whole_coordinate_range(eps, wide):
    """The random mode draws its positions from [1000, 1315) x [5000, 5315), every 40th segment within 44 of either end of the 32-bit
    range: bit 31 is set only next to 2^32.  `whole` draws the centres from the whole range, every eighth segment around 2^31 with
    its jitter across the top bit: about half of the coordinates have the top bit set (the program counts them)."""
    assert os.path.exists(SEG), "run `make harness`"
    r = subprocess.run([SEG, "20000", "2", str(wide), str(eps), "whole"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"eps {eps}" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
    top, of = (int(x) for x in re.search(r"(\d+) of (\d+) coordinates with the top bit set", r.stdout).groups())
    assert 0.3 * of < top < 0.7 * of, r.stdout[-300:]


def _sort_check(*args):
    assert os.path.exists(SORT), "run `make harness`"
    r = subprocess.run([SORT, "check"] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "check: 0 mismatches" in r.stdout, r.stdout[-1500:] + r.stderr[-500:]


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [28, 32])
@pytest.mark.parametrize("keys", ["equal", "two", "asc", "desc", "skew90", "low_digit_const", "top_digit_const"])
def test_radix_sort_on_skewed_keys(keys, bits):
    """Tiles in which every key has the same digit, digits that alternate by lane, sorted and reversed input, a pass with one occupied
    bin: 1 000 003 records (196 tiles, the last one partial) against std::stable_sort, payload high halves included."""
    _sort_check(keys, 1000003, bits)


@pytest.mark.gpu
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("g,t", [(0, 8), (0, 16), (1, -8), (1, -1), (1, 0), (1, 1), (2, 0), (2, 8)])
def test_radix_sort_tile_counts_around_the_persistent_grid(g, t, delta):
    """n = (g * G + t) tiles + delta records, G = sort_scatter's persistent grid (the program prints it): the XCD tile order with one
    tile per XCD, the plain stride, exactly full rounds, a last round with idle blocks, a last tile that is full and one of one record."""
    _sort_check("uniform", f"g{g}:{t}:{delta}", 28)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3 * 5120 + 17, 1000003])
@pytest.mark.parametrize("key_offset", [1, 2, 3])
def test_radix_sort_unaligned_views(key_offset, n):
    """Key arrays that start 1, 2, 3 elements into their allocation (payload arrays 1): sort_hist's scalar loads on full tiles; the
    guard words around all four arrays stay as they were."""
    _sort_check("uniform", n, 28, 0, key_offset)


@pytest.mark.gpu
@pytest.mark.parametrize("first_bit,bits", [(7, 14), (29, 3)])
def test_radix_sort_of_a_bit_field(first_bit, bits):
    """first_bit > 0 (the sharded build sorts 1 to 3 owner bits at a shift): random 32-bit keys, stable by the field alone, the other bits
    carried along untouched."""
    _sort_check("uniform", 1000003, bits, first_bit)
    _sort_check("uniform", 5120 * 9 + 1, bits, first_bit, 3)
