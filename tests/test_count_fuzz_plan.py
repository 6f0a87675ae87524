"""What the count-table fuzz (tests/test_gpu_count_fuzz.py) will do, checked without a GPU: the coverage of the default seed set, read off
count_fuzz_np.plan alone, and the non-vacuity of its inputs, read off the reference chain count_fuzz_np.host_pipeline alone."""
import collections

import numpy as np
import pytest

from tests import count_fuzz_np as F

SEEDS = range(F.N_DEFAULT)


@pytest.fixture(scope="module")
def plans():
    return [F.plan(s) for s in SEEDS]


def test_plan_is_a_pure_function_of_the_seed():
    assert all(F.plan(s) == F.plan(s) for s in (0, 7, 30))
    a, b = F.reads_of(F.plan(5)), F.reads_of(F.plan(5))
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_coverage_of_the_default_seeds(plans):
    ks = collections.Counter(p.k for p in plans)
    assert set(ks) == set(F.KS) and 32 not in ks and 1 not in ks
    assert all(ks[k] >= 2 for k in F.KS), ks
    layouts = collections.Counter(n for p in plans for n in p.layout_names())
    assert all(layouts[n] >= 4 for n in F.LAYOUTS), layouts
    first = collections.Counter(p.layouts[0].name for p in plans)
    assert all(first[n] >= 1 for n in F.LAYOUTS), first            # the chain itself starts from every layout
    for two in (False, True):
        mine = [p for p in plans if p.two == two]
        assert {n for p in mine for n in p.layout_names()} == set(F.LAYOUTS), two
        assert {p.stream for p in mine} == {"side", "default"}, two
        assert any(p.has_long for p in mine), two
    assert all(p.stream == ("side" if p.seed % 2 else "default") for p in plans)
    assert {p.layouts[i].uniform for p in plans for i in range(len(p.layouts)) if p.layouts[i].name == "misaligned"} == {False, True}
    assert all(1 <= l.lead <= 15 for p in plans for l in p.layouts if l.name == "misaligned")


def test_the_reads_are_what_the_plan_says(plans):
    for p in plans:
        reads = F.reads_of(p)
        lens = np.array([len(r) for r in reads])
        assert 150 <= len(reads) == p.n_reads <= 600 and 1500 <= p.genome_len <= 6000
        names = {x[0] for x in p.pieces}
        assert names == {"repeat", "variant", "hairpin", "homopolymer", "tip", "graft", "circle"}
        assert all(x[3] > p.k for x in p.pieces if x[0] == "repeat") and all(x[2] > p.k for x in p.pieces if x[0] in ("hairpin", "homopolymer"))
        if p.length_mode == "one":
            assert (lens == p.read_len).all() and (p.read_len in F.ONE_LENGTHS or 300 <= p.read_len <= 1200)
        else:
            assert (lens == 0).any() and ((lens > 0) & (lens < p.k)).any()
            assert sorted(lens[lens > 260].tolist()) == sorted(p.long_lens) and all(300 <= x <= 1200 for x in p.long_lens)
        assert int(lens.max()) == p.longest
        both = np.concatenate(reads)
        assert (both == ord("N")).any() and ((both >= ord("a")) & (both <= ord("t"))).any()
        assert (~np.isin(both, np.frombuffer(b"ACGTacgtN", np.uint8))).any(), p.seed
        for l, buf, lead, nbytes, offsets in F.handovers(p, reads):
            assert (offsets is None) == l.uniform and len(buf) == 2 * F.GUARD_BYTES + lead + nbytes
            route_long = l.bound > 256
            assert route_long == (l.name in ("uniform_long", "ragged_long")) or l.name == "misaligned", (p.seed, l)


def test_the_reference_chain_has_structure_in_every_stage(plans):
    """run on every default seed: a stage that is vacuous for a seed is still compared on the device, but over the seed set each
    stage must have something to get wrong in at least three quarters of the seeds, and links and multi-segment reads in all"""
    seen = collections.Counter()
    for p in plans:
        reads = F.reads_of(p)
        s = F.structure(p, F.host_pipeline(p, reads), reads)
        assert s["link"] and s["multi_segment_read"], (p.seed, s)
        seen.update(name for name, ok in s.items() if ok)
    need = -(-3 * len(plans) // 4)
    assert all(seen[name] >= need for name in ("fork", "link", "cleaned", "two_components", "multi_segment_read", "support_0_and_many",
                                               "corrected", "selected")), (seen, need)
