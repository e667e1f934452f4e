"""CPU tests of one shard of a certificate-groups call (narwhal-tusk_amd/csrc/group_plan.hpp,
compiled into the host harness) against a plain numpy model: the chunk bases, the
(chunk, signature) -> verdict-bit map, the merge of the registry misses' fallback
verdicts, and the scatter of the shard's signature bits into the caller's bitmap."""
import ctypes

import numpy as np
import pytest

import _hostarith

U64P, U32P, U8P = (ctypes.POINTER(t) for t in (ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint8))


def _p(a, t=U64P):
    return a.ctypes.data_as(t)


class Shard:
    """groups [glo, ghi) of (first, cnt) under `targets`, planned by the harness"""

    def __init__(self, glo, ghi, first, cnt, targets):
        self.glo, self.ghi, self.first, self.cnt = glo, ghi, first, cnt
        self.tg = (ctypes.c_ulonglong * len(targets))(*targets)
        self.nt = len(targets)
        ends, E, W = (np.zeros(65, np.uint64) for _ in range(3))
        self.start = np.zeros(ghi - glo + 1, np.uint64)
        scal = np.zeros(5, np.uint64)
        self.C = _hostarith.load().nth_group_plan(*self.head(), _p(ends), _p(E), _p(W), _p(self.start), _p(scal), 64)
        self.ends = [int(x) for x in ends[:self.C]]
        self.E, self.W = E[:self.C + 1].astype(np.int64), W[:self.C + 1].astype(np.int64)
        self.m, self.sw, self.gw, self.max_chunk, self.direct = (int(x) for x in scal)
        self.bits = np.zeros(max(self.m, 1), np.uint64)
        _hostarith.load().nth_group_bits(*self.head(), _p(self.bits))
        self.bits = self.bits[:self.m].astype(np.int64)

    def head(self):
        return (ctypes.c_ulonglong(self.glo), ctypes.c_ulonglong(self.ghi), _p(self.first), _p(self.cnt, U32P),
                self.tg, self.nt)


def _layouts(rng, G):
    """(first, cnt) dense, and reversed with three unused slots between neighbours"""
    cnt = rng.integers(0, 30, G).astype(np.uint32)
    if G > 80:
        cnt[[3, 77]] = 0
    dense = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint64)
    scat = np.zeros(G, np.uint64)
    pos = 0
    for g in range(G - 1, -1, -1):
        scat[g] = pos
        pos += int(cnt[g]) + 3
    return cnt, dense, scat


def _cases():
    for G in (1, 63, 64, 65, 203, 1000):
        for glo in sorted({0, ((G - 1) // 64 + 1) // 2 * 64}):  # shard starts are multiples of 64 groups
            for nchunks in (1, 3, 15):
                yield G, glo, nchunks


@pytest.mark.parametrize("G,glo,nchunks", list(_cases()))
def test_group_shard_plan_merge_scatter(G, glo, nchunks):
    rng = np.random.default_rng(1000 * G + 10 * glo + nchunks)
    cnt, dense, scat = _layouts(rng, G)
    c64 = cnt.astype(np.int64)
    total = int(c64[glo:].sum())
    targets = [max(64, total // nchunks // 64 * 64)] * (nchunks - 1) + [max(total, 1)]
    for first in (dense, scat):
        s = Shard(glo, G, first, cnt, targets)
        # the plan: whole group words per chunk, bases and starts as a running sum
        assert s.ends[-1] == G and all((e - glo) % 64 == 0 for e in s.ends[:-1]) and 1 <= s.C <= nchunks
        lo = [glo] + s.ends[:-1]
        mc = [int(c64[a:b].sum()) for a, b in zip(lo, s.ends)]
        assert list(np.diff(s.E)) == mc and list(np.diff(s.W)) == [(x + 63) // 64 for x in mc]
        assert (s.m, s.sw, s.gw, s.max_chunk) == (total, int(s.W[-1]), (G - glo + 63) // 64, max(mc))
        want_start = np.concatenate([np.cumsum(c64[a:b]) - c64[a:b] for a, b in zip(lo, s.ends)])
        assert np.array_equal(s.start[:G - glo].astype(np.int64), want_start)
        f = first.astype(np.int64)
        assert s.direct == (total > 0 and bool(np.all(f[glo + 1:G] == f[glo:G - 1] + c64[glo:G - 1])))
        # every signature a distinct bit, inside its chunk's own words
        assert len(np.unique(s.bits)) == s.m
        at = 0
        for c in range(s.C):
            b = s.bits[at:at + mc[c]]
            assert np.array_equal(b, 64 * s.W[c] + np.arange(mc[c]))
            at += mc[c]
        if s.m == 0:
            continue
        # merge: verdicts with the misses rejected, then the fallback's verdicts for them
        gidx = np.repeat(np.arange(glo, G), c64[glo:])           # group of signature e (group order)
        tidx = np.arange(s.m) - np.repeat(np.cumsum(c64[glo:]) - c64[glo:], c64[glo:])
        truth = rng.random(s.m) < 0.9
        missed = rng.random(s.m) < 0.2
        fallback = rng.random(int(missed.sum())) < 0.7

        def words(sig_ok):
            sb = np.zeros(s.sw + 1, np.uint64)
            np.bitwise_or.at(sb, s.bits[sig_ok] >> 6, np.uint64(1) << (s.bits[sig_ok] & 63).astype(np.uint64))
            bad = np.zeros(G - glo, bool)
            bad[gidx[~sig_ok] - glo] = True
            gb = np.packbits(~bad, bitorder="little")
            gb = np.concatenate([gb, np.zeros(8 * s.gw - len(gb), np.uint8)]).view(np.uint64).copy()
            return sb, gb

        sb, gb = words(truth & ~missed)
        final = truth.copy()
        final[missed] = fallback
        mw = np.packbits(fallback, bitorder="little")
        mw = np.concatenate([mw, np.zeros(8 * ((len(fallback) + 63) // 64 + 1) - len(mw), np.uint8)]).view(np.uint64)
        mg = np.ascontiguousarray(gidx[missed].astype(np.uint64))
        mt = np.ascontiguousarray(tidx[missed].astype(np.uint32))
        _hostarith.load().nth_group_merge(*s.head(), _p(mg), _p(mt, U32P), ctypes.c_ulonglong(len(mg)), _p(mw), _p(sb),
                                          _p(gb))
        want_sb, want_gb = words(final)
        assert np.array_equal(sb, want_sb) and np.array_equal(gb, want_gb)
        # scatter: signature t of group g at first[g] + t and nowhere else
        nsig = int((f + c64).max())
        out = np.zeros((nsig + 7) // 8 + 1, np.uint8)
        _hostarith.load().nth_group_scatter(*s.head(), _p(sb), _p(out, U8P))
        want = np.zeros(8 * len(out), bool)
        want[f[gidx] + tidx] = final
        assert np.array_equal(np.unpackbits(out, bitorder="little").astype(bool), want)
