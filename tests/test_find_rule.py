"""tests/find_rule.py — the numpy statement of PABruijnGraph::findAll that tests/test_gpu_find.py holds pag_find_all_batch to —
on strings made by hand, and its node table against the one tests/succ_rule.py reads from the same dumps."""
import os
import subprocess

import numpy as np
import pytest

import find_rule
import goldens
import succ_rule


def test_codes_forward_and_reverse():
    # first base most significant: ACGT = 0 1 2 3 -> 0b00011011
    assert find_rule.codes("ACGT", 4).tolist() == [0b00011011]
    assert find_rule.codes("ACGTA", 4).tolist() == [0b00011011, 0b01101100]
    # the reverse strand is the complement read back to front: of AACG it is CGTT
    assert find_rule.codes("AACG", 4, reverse=True).tolist() == find_rule.codes("CGTT", 4).tolist()
    assert find_rule.codes("AACGG", 3, reverse=True).tolist() == find_rule.codes("CCGTT", 3).tolist()
    # a palindrome reads the same in both strands
    for s, k in (("ACGT", 4), ("AACGTT", 3), ("GAATTC", 2), ("ACGTACGT", 5)):
        assert find_rule.codes(s, k, reverse=True).tolist() == find_rule.codes(s, k).tolist()
    # k = 16 uses all 32 bits
    assert find_rule.codes("T" * 16, 16).tolist() == [0xFFFFFFFF] and find_rule.codes("G" + "A" * 15, 16).tolist() == [0x80000000]


def test_what_is_no_base_is_a():
    k = 5
    assert find_rule.codes("N" * 9, k).tolist() == [0] * 5
    # ... in the packed sequence, so the reverse strand reads T there
    assert find_rule.codes("N" * 9, k, reverse=True).tolist() == [4 ** k - 1] * 5
    assert find_rule.codes("ACNNT", k).tolist() == find_rule.codes("ACAAT", k).tolist()
    packed, byte_off, lengths = find_rule.pack(["NNNN", "ACGTN", ""])
    assert packed.tolist() == [0, 0, 0, 0, 0b11100100, 0, 0, 0] and byte_off.tolist() == [0, 4, 8] and lengths.tolist() == [4, 5, 0]


def test_lengths_around_k():
    k = 4
    table = find_rule.make_table([0b00011011, 0b01101100], [2, 1], [(7 << 32) | 9, (7 << 32) | 30, 5], [3, 1, 65535])
    solid = np.array([0, 0b00011011, 0b01101100], dtype=np.uint32)
    seqs = ["ACG", "ACGT", "ACGTA", "AAAA", "TTTT", ""]
    hit_off, hits, vert = find_rule.find_all(table, solid, k, seqs)
    assert hit_off.tolist() == [0, 0, 1, 3, 4, 4, 4]
    assert hits["offset"].tolist() == [0, 0, 1, 0] and hits["code"].tolist() == [0b00011011, 0b00011011, 0b01101100, 0]
    # a solid k-mer nothing was placed on is a hit without vertices; first runs over the whole call
    assert hits["n_pos"].tolist() == [2, 2, 1, 0] and hits["first"].tolist() == [0, 2, 4, 5]
    assert vert["pos"].tolist() == [(7 << 32) | 9, (7 << 32) | 30] * 2 + [5] and vert["abundance"].tolist() == [3, 1, 3, 1, 65535]
    # the reverse strand of ACGTA is TACGT: ACGT at offset 1
    hit_off, hits, vert = find_rule.find_all(table, solid, k, ["ACGTA"], [True])
    assert hit_off.tolist() == [0, 1] and hits["offset"].tolist() == [1] and hits["n_pos"].tolist() == [2]
    # every k-mer solid: every offset is a hit
    hit_off, hits, vert = find_rule.find_all(table, None, k, ["ACGTACG"])
    assert hits["offset"].tolist() == [0, 1, 2, 3] and hits["n_pos"].tolist() == [2, 1, 0, 0]
    # no sequence at all, no node at all
    hit_off, hits, vert = find_rule.find_all(table, solid, k, [])
    assert hit_off.tolist() == [0] and len(hits) == 0 and len(vert) == 0
    empty = find_rule.make_table([], [], [], [])
    hit_off, hits, vert = find_rule.find_all(empty, solid, k, ["ACGT"])
    assert hits["n_pos"].tolist() == [0] and len(vert) == 0


def test_solid_set_of_a_file_s_words():
    # the header word k is a code like the others; what is no k-mer code can never be found
    assert find_rule.solid_of_words([5, 1000, 3, 4 ** 5, 3, 2 ** 40], 5).tolist() == [3, 5, 1000]


def test_host_half_of_the_call_under_sanitizers():
    """csrc/hip/find_plan.hpp (the sequences' descriptors checked, the offsets cut into tiles) in tests/harness/find_plan_main.cpp, a
    program of its own built with -fsanitize=address,undefined: the tilings the GPU test searches and lengths 0 and 2^32 - 1"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "harness", "bin", "find_plan_sanitized")
    subprocess.run(["make", "-C", root, exe[len(root) + 1:]], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


@pytest.mark.parametrize("name", goldens.case_names())
def test_node_table_equals_succ_rule_s(name):
    mine, theirs = find_rule.node_tables(name), succ_rule.load_graph(name)
    assert len(mine) == len(theirs) > 0
    for t, g in zip(mine, theirs):
        order = np.argsort(g["code"], kind="stable")
        assert np.array_equal(t["code"], g["code"][order])
        n_pos = np.diff(g["pos_off"])
        assert np.array_equal(np.diff(t["pos_off"]), n_pos[order])
        assert n_pos.min() >= 1, "the dump skips nodes without positions"
        pos = (g["ctg"].astype(np.uint64) << np.uint64(32)) | g["ref"].astype(np.uint64)
        take = np.concatenate([np.arange(g["pos_off"][n], g["pos_off"][n + 1]) for n in order])
        assert np.array_equal(t["pos"], pos[take])
        assert len(t["cnt"]) == len(pos) and t["cnt"].min() >= 1 and t["cnt"].max() <= 0xFFFF
