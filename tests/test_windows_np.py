"""tests/windows_np.py on the CPU: its arm table against its own cases, the sizes of the batches, the proof that no case of
tests/test_gpu_windows_sweep.py could pass with a kernel that mishandles the units past its first launch, the numpy slot rule against
the oracle, and the conditions on the inputs (invalid bytes, the fixed reads, the footprint)."""
import time

import numpy as np
import pytest

from tests import elem_np as E
from tests import windows_np as M

EVERY = M.CASES + M.EDGE + M.DIRTY_THEN_CLEAN + M.REPEAT


# ------------------------------------------------------------------ the arms

def test_every_arm_has_a_case():
    named = {a for c in M.CASES for a in c.arm.names if not a.startswith("zero<")}
    named |= {c.arm.zero for c in M.CASES if c.zero}
    assert named == set(M.ARMS), (sorted(set(M.ARMS) - named), sorted(named - set(M.ARMS)))
    assert len({c.id for c in M.CASES}) == len(M.CASES) and len(set(M.ARMS)) == len(M.ARMS)
    for c in EVERY:
        a = M.arm_of(c.call, c.k, c.L, c.ragged, c.lead, c.want, c.flags_shift, c.words_shift)
        assert a == c.arm and a.name in c.id
    # the edge-only arm is what the edge sizes below 64 reads reach
    assert M.arm_of("windows2", 33, 47, False, 0, M.ALL4, n=63).name == "generic2[n<64]" and "generic2[n<64]" in M.EDGE_ONLY
    assert any(c.call == "windows2" for c in M.EDGE) and {1, 63} <= set(M.SIZES)
    # each uniform one-word sink and frame from an aligned base and from a misaligned one
    for sink in ("ring", "sinkflags", "staged"):
        for nw in (10, 16):
            leads = {c.lead != 0 for c in M.CASES if any(a.startswith(f"{sink}<{nw},") for a in c.arm.names)}
            assert leads == {False, True}, (sink, nw)
    assert {c.lead != 0 for c in M.CASES if c.arm.name.startswith("w2<") and not c.ragged and c.arm.unit == "tile"} == {False, True}


def test_shapes_are_the_smallest_that_reach_the_arm():
    for c in M.CASES:
        a, W = c.arm, c.L - c.k + 1
        if a.unit == "read":
            assert c.longest <= 24 or "L=" in a.name or "L>" in a.name or c.call == "windows2", c.id
        elif a.unit == "segtile":
            assert 257 <= c.L <= 300, c.id
        elif c.zero:
            # (the 16-word uniform frame: no read shorter than 161 bases reaches it, the largest k leaves the fewest windows)
            assert c.short or W == 1 or (c.L == 161 and c.k == (64 if c.call == "windows2" else 31) and c.want == ("flags",)), c.id
        elif "<16," in a.name:
            assert 161 <= c.longest <= 176 and (c.ragged or len(c.want) == 1 or c.want == ("canon", "flags")), c.id
        else:
            assert 40 <= c.longest <= 70, c.id
        if a.name.startswith("ring<") and not c.zero:
            assert W > 32, c.id           # the ring wraps
        if a.unit != "tile" or "<16," in a.name:
            assert c.want != M.ALL4 or c.longest <= 48, c.id


def test_arm_routing_thresholds():
    a = lambda *x, **kw: M.arm_of(*x, **kw).name
    assert a("windows", 31, 150, False, 0, ("canon",)) == "ring<10,k>=18>"
    assert a("windows", 31, 158, False, 0, ("canon",)) == "staged<10,k>=18,nt>"              # W = 128
    assert a("windows", 31, 150, False, 0, M.ALL4) == "ring<10,k>=18>+ring<10,k>=18>+ring<10,k>=18>+sinkflags<10,k>=18>"
    assert a("windows", 31, 150, False, 0, M.ALL4, flags_shift=1) == "staged<10,k>=18,nt>"    # W = 120
    assert a("windows", 31, 150, False, 0, ("flags",)) == "sinkflags<10,k>=18>"
    assert a("windows", 31, 61, False, 0, M.ALL4) == "staged<10,k>=18,plain>"                 # W = 31 < 32
    assert a("windows", 16, 160, False, 0, ("fw",)) == "ring<10,k<=16>" and a("windows", 17, 161, False, 0, ("fw",)) == "ring<16,k=17>"
    assert a("windows", 31, 160, False, 1, ("fw",)) == "generic1[L=160,misaligned]" and a("windows", 31, 159, False, 1, ("fw",)) == "ring<10,k>=18>"
    assert a("windows", 31, 160, True, 0, ("fw",)) == "rring<10,k>=18>" and a("windows", 31, 0, True, 0, ("fw",)) == "rring<16,k>=18>"
    assert a("windows", 31, 256, True, 0, ("fw", "flags")) == "rstaged<16,k>=18>"
    assert a("windows", 31, 256, True, 0, ("fw", "rc", "flags")) == "rring<16,k>=18>+rstaged<16,k>=18>"
    assert M.arm_of("windows", 31, 257, True, 0, ("fw",)).plan == "seg_ragged" and a("windows", 31, 257, True, 4, ("fw",)) == "generic1[L>256,misaligned]"
    assert a("windows", 1, 257, False, 0, ("fw",)) == "generic1[k=1]"
    assert a("windows2", 33, 160, False, 0, ("fw", "rc")) == "w2<10,STAGE,uniform>+w2<10,STAGE,uniform>"
    assert a("windows2", 33, 161, False, 0, ("flags",)) == "w2<16,FLAGS,uniform>"
    assert a("windows2", 64, 64, True, 0, ("canon",)) == "w2<10,STAGE,ragged>" and a("windows2", 64, 0, True, 0, ("canon",)) == "w2<16,STAGE,ragged>"
    assert a("windows2", 64, 150, True, 0, ("canon",), words_shift=8) == "generic2[words misaligned]"
    assert a("windows2", 64, 150, True, 0, ("flags",), words_shift=8) == "w2<10,FLAGS,ragged>"
    assert a("windows2", 33, 257, False, 0, ("canon",), n=31) == "generic2[n<64]" and a("windows2", 33, 257, False, 0, ("canon",), n=32) == "w2<16,STAGE,segments>"
    assert a("windows2", 33, 300, True, 0, ("canon",), n=63, n_seg=64) == "w2<16,STAGE,segments>" and a("windows2", 33, 300, True, 0, ("canon",), n=70, n_seg=63) == "generic2[n<64]"
    assert M.segments_per_read(257, 31) == 2 and M.segments_per_read(1000, 31) == 5 and M.segments_per_read(300, 9) == 2
    assert list(M.seg_count([0, 30, 31, 256, 257, 300, 600], 31)) == [0, 0, 1, 1, 2, 2, 3]


# ------------------------------------------------------------------ the slot rule

def test_slot_rule_equals_the_oracle(orc):
    """200 random small batches, uniform and ragged, both widths, invalid bytes of every kind"""
    rng = np.random.default_rng(11)
    for i in range(200):
        two, ragged = bool(i & 1), bool(i & 2)
        k = int(rng.integers(33, 65)) if two else int(rng.integers(1, 32))
        n = int(rng.integers(1, 9))
        lens = rng.integers(0, k + 20, n) if ragged else np.full(n, int(rng.integers(k, k + 20)))
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        host = np.frombuffer(b"ACGTacgt", np.uint8)[rng.integers(0, 8, int(off[-1]))].copy()
        bad = rng.random(len(host)) < (0.0, 0.01, 0.05)[i % 3]
        host[bad] = np.frombuffer(b"NnX\n\x00@", np.uint8)[rng.integers(0, 6, int(bad.sum()))]
        fn = orc.canonical_windows2 if two else orc.canonical_windows
        want = fn(host, n, 0 if ragged else int(lens[0]), k, offsets=off if ragged else None)
        win = orc.win_offsets_for(n, int(lens[0]), k, off if ragged else None)
        got = M.windows_np(host, off[:-1], lens, win, k)
        for nm, g, w in zip(M.NAMES, got, want):
            assert E.same(g, w), (i, k, nm)


# ------------------------------------------------------------------ the cases are large enough, dirty enough and small enough

@pytest.fixture(scope="module")
def built(orc):
    cache = {}

    def get(c, n_cu, **kw):
        key = (c, n_cu, tuple(sorted(kw.items())))
        if key not in cache:
            if len(cache) > 3:
                cache.clear()
            cache[key] = M.build(c, n_cu, oracle=orc, **kw)
        return cache[key]
    return get


@pytest.mark.parametrize("n_cu", [8, 256])
def test_cases_could_not_pass_with_a_broken_kernel(built, n_cu):
    cost, biggest = {}, (0, "")
    for c in M.CASES:
        t0 = time.perf_counter()
        b = built(c, n_cu)
        U = (512 if c.zero else c.arm.per_cu) * n_cu
        assert b.U == U and U < M.past(U) <= b.units < 2 * U, (c.id, b.units)
        assert b.n % 64 != 0 and b.period > -(-b.n // 64) and all(b.period % d for d in range(2, 64)), c.id
        # ---- poison occurs in no expected array
        for nm in c.want:
            assert not (b.exp[nm] == (M.POISON_U8 if nm == "flags" else M.POISON_U64)).any(), (c.id, nm)
        # ---- the three broken kernels
        R0 = b.first_read_of_unit(U)
        assert int(b.unit_of_read(R0)) == U and (R0 == 0 or int(b.unit_of_read(R0 - 1)) == U - 1), c.id
        ranges = M.late_ranges(b)
        assert ranges[0][0] == R0 and ranges[-1][1] == b.n and len(ranges) >= min(b.units - U, 64), c.id
        seen = {"stops": 0, "previous": 0, "elsewhere": 0, "moved": 0}
        for r0, r1 in ranges:
            diff = {key: False for key in seen}
            for nm in c.want:
                want, stops, previous, elsewhere, (src, moved) = M.faulty(b, nm, r0, r1)
                diff["stops"] |= bool((stops != want).any())
                diff["previous"] |= bool((previous != want).any())
                diff["elsewhere"] |= bool((elsewhere != want).any())
                diff["moved"] |= bool((moved != src).any())
            for key in seen:
                seen[key] += diff[key]
        # every unit looked at that owns a slot differs under every fault (a run of reads all shorter than k owns none)
        owning = sum(int(b._at(b.win, r1)) > int(b._at(b.win, r0)) for r0, r1 in ranges)
        assert owning >= len(ranges) - (2 if c.ragged else 0) and owning > 0, c.id
        assert seen["stops"] == seen["previous"] == seen["elsewhere"] == owning, (c.id, seen, owning)
        # (`elsewhere` equals `stops` on the unit's own slots; what it adds is `moved`, the earlier unit's slots holding this unit's
        # words -- which shows wherever both units own a slot: all but, at most, one run of ragged reads shorter than k)
        assert seen["moved"] >= owning - 1, (c.id, seen)
        # ---- the input: an invalid byte in under 1 % of the reads and over 10 % of the tiles; the fixed reads
        td = b.tile_dirty()
        late = b.dirty_reads()[R0:]
        assert b.dirty.mean() < 0.01 and td.mean() > 0.10 and late.any() and not late.all(), (c.id, b.dirty.mean(), td.mean())
        codes_ok = E.base_codes(b.bases)[1]
        o = b.off
        assert not codes_ok[o[1]: o[2]].any() and o[2] > o[1] and not codes_ok[o[2]] and not codes_ok[o[4] - 1] and o[4] > o[3], c.id
        last = (b.n - 1) % b.period
        assert last >= 8 and not codes_ok[o[last]: o[last + 1]].all(), c.id
        bad_reads = np.add.reduceat(~codes_ok, o[:-1][b.lens > 0]) > 0
        assert (bad_reads == b.dirty[b.lens > 0]).all(), c.id
        if c.ragged:
            assert (b.lens[4], b.lens[5], b.lens[6]) == (0, c.k - 1, c.longest) and b.lens.max() == c.longest, c.id
        else:
            assert (b.lens == c.L).all()
        biggest = max(biggest, (b.footprint(), c.id))
        cost[c.id] = time.perf_counter() - t0
    slowest = max(cost, key=cost.get)
    print(f"\nn_cu = {n_cu}: {sum(cost.values()):.1f} s for {len(cost)} builds, the slowest {slowest}: {cost[slowest]:.2f} s; "
          f"the largest footprint {biggest[0] / 2**20:.0f} MiB: {biggest[1]}")
    assert biggest[0] < M.CAP_BYTES, biggest
    if n_cu == 256:
        assert biggest[0] > M.CAP_BYTES // 4          # (the cap is not a loose one)


def test_the_repeated_block_is_the_oracle_on_the_whole_batch(built, orc):
    """n_cu = 8, every case: bases, offsets and expected arrays of the whole batch from the block, against the oracle (and the numpy
    slot rule) on all of it"""
    for c in M.CASES:
        b = built(c, 8)
        host, off, win = b.host_bases(), b.host_offsets(), b.host_win_offsets()
        assert len(host) == b.total_bytes == int(off[-1]) and int(win[-1]) == b.total
        if not c.ragged:
            assert (off == np.arange(b.n + 1, dtype=np.uint64) * np.uint64(c.L)).all()
        fn = orc.canonical_windows2 if b.two else orc.canonical_windows
        want = dict(zip(M.NAMES, fn(host, b.n, c.L, c.k, offsets=off if c.ragged else None)))
        assert (orc.win_offsets_for(b.n, c.L, c.k, off if c.ragged else None) == win).all()
        for nm in c.want:
            assert E.same(b.expected(nm), np.ascontiguousarray(want[nm]).reshape(-1)), (c.id, nm)
        # a slot's read and unit, as a failure reports them
        for s in (0, b.total // 2, b.total - 1):
            r, t, late = b.where(s)
            assert win[r] <= s < win[r + 1] and t == int(b.unit_of_read(r)) and late == (t >= b.U), (c.id, s)
        assert b.where(b.total - 1)[2]


def test_edge_sets(built):
    fam = {(c.call, c.ragged, c.arm.unit) for c in M.EDGE}
    assert fam >= {(call, rg, "tile") for call in ("windows", "windows2") for rg in (False, True)}
    assert fam >= {("windows", False, "segtile"), ("windows2", False, "segtile"), ("windows", False, "read"), ("windows2", True, "read")}
    for c in M.EDGE:
        for size in M.SIZES:
            b = built(c, 8, size=size)
            if size == "U":
                assert b.units == b.U and b.first_read_of_unit(b.U) == b.n, (c.id, b.units, b.n)
            else:
                assert b.n == size
            assert b.total == int(b.host_win_offsets()[-1])


def test_clean_batches_are_clean(built):
    for c in M.DIRTY_THEN_CLEAN:
        assert c in M.CASES and c.arm.zero
        b = built(c, 8, clean=True)
        assert E.base_codes(b.bases)[1].all() and not b.dirty.any() and b.n == built(c, 8).n
    assert {c.call for c in M.DIRTY_THEN_CLEAN} == {"windows", "windows2"} and any(c.zero for c in M.DIRTY_THEN_CLEAN)
    assert [c.arm.name.split("<")[0] for c in M.REPEAT] == ["ring", "w2"] and "STAGE" in M.REPEAT[1].arm.name and all(c in M.CASES for c in M.REPEAT)
