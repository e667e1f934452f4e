"""TEST INFRASTRUCTURE (not a test module): what tests/test_gpu_passes.py, the added tests of
tests/test_gpu_signer.py and tests/_variant_probe.py share -- contexts created under launch-geometry
variables, the proof that a variable took effect, and the batches with their expected verdicts.

The grid-stride kernels size their grids from the context's figures (Device::init, csrc/runtime.hpp):
  k_ed25519_verify   at most ws_slots blocks (NT_WS_SLOTS, else NT_GRID_CUS x occupancy x 4), each block
                     iteration 256 lanes x 2 signatures (the device API and the group calls) or x 1 (a
                     verify_strict chunk of at most one round)
  k_ed25519_sign, k_signer_digests   at most sign_blocks = CUs x 8 blocks of 256
  k_signer_votes     at most sign_blocks x 4 rows of 64
so a context made for one slot, or one CU, runs the later passes of those loops at a few thousand items."""
import contextlib
import os
import types

import numpy as np

import ntcrypto

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# every variable a context of these tests is made under; the ones a test does not name are unset
KNOBS = ("NT_WS_SLOTS", "NT_GRID_CUS", "NT_BCOMB_BITS", "NT_KTAB_KEYS", "NT_XCACHE_SLOTS", "NT_KEYSET_COMB_BITS",
         "NT_PIPE_CHUNKS", "NT_PIPE_ROUND", "NT_SLOTS", "NT_HBM_BUDGET", "NT_KEY_CACHE")
VERIFY_OCC = 2            # the verify kernel's default waves per SIMD: ws_slots = CUs x VERIFY_OCC x 4
DEV_PER_BLOCK = 512       # signatures per block iteration, two per lane
HOST_PER_BLOCK = 256      # ... one per lane
SIGN_PER_CU = 8 * 256     # signatures (k_ed25519_sign, k_signer_digests) and votes (32 rows of 64) per pass and CU


def passes(n, per_block, blocks):
    """iterations of the grid-stride loop that the busiest block of a launch over n items runs"""
    return -(-(-(-n // per_block)) // blocks)


@contextlib.contextmanager
def environment(**env):
    """os.environ with KNOBS unset but for `env`, restored on exit (libntcrypto reads these per context or per
    launch, so a test sets them around nt_init and its calls)"""
    saved = {k: os.environ.get(k) for k in set(KNOBS) | set(env)}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        for k, v in env.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def corpus():
    d = np.load(os.path.join(GOLD, "ed25519_corpus.npz"))
    return {k: d[k] for k in d.files}


def workspace_after_four(be, c):
    """bytes of [k]A workspace the context holds after one 4-signature verify_strict: the slot that took the
    call grew lane 0's workspace to its full ws_slots slots (verify_tables), nothing else has one yet"""
    assert be.memory_info()["workspace_bytes"] == 0
    got = be.verify_strict(c["pk"][:4], c["sig"][:4], c["msg"], c["off"][:4], c["len"][:4])
    assert np.array_equal(got, c["strict"][:4].astype(bool))
    return be.memory_info()["workspace_bytes"]


def slot_bytes(c):
    """bytes of one workspace slot, from a context of one slot"""
    with environment(NT_WS_SLOTS=1):
        be = ntcrypto.Backend(device=0)
        try:
            b = workspace_after_four(be, c)
        finally:
            be.close()
    assert b > 0 and b % 4096 == 0
    return b


@contextlib.contextmanager
def context(c, per_slot, slots, **env):
    """A fresh context under `env` that provably has `slots` workspace slots (so the variable was read: a test
    that passes with it ignored proves nothing).  The environment stays set for the body: NT_KTAB_KEYS,
    NT_XCACHE_SLOTS, NT_PIPE_CHUNKS and NT_KEYSET_COMB_BITS are read per launch or per key set."""
    with environment(**env):
        be = ntcrypto.Backend(device=0)
        try:
            got = workspace_after_four(be, c)
            assert got == slots * per_slot, (env, got, slots, per_slot)
            yield be
        finally:
            be.close()


class Batch:
    """n (key, signature, message slice) items and their expected verdicts"""

    def __init__(self, pk, sig, msg, off, ln, strict, cofactorless):
        self.pk, self.sig, self.msg = pk, sig, msg
        self.off, self.ln = np.asarray(off, np.uint64), np.asarray(ln, np.uint64)
        self.strict, self.cofactorless = np.asarray(strict, bool), np.asarray(cofactorless, bool)
        self.n = len(pk)

    def args(self):
        return self.pk, self.sig, self.msg, self.off, self.ln


def batch_x(c, reps=8):
    """the 360-entry corpus (small-order, mixed-order, non-canonical and off-curve keys and R) tiled: labels"""
    return Batch(np.tile(c["pk"], (reps, 1)), np.tile(c["sig"], (reps, 1)), c["msg"], np.tile(c["off"], reps),
                 np.tile(c["len"], reps), np.tile(c["strict"], reps), np.tile(c["batch_rule"], reps))


def batch_y(orc, n=3000, nkeys=200, seed=4711):
    """n signatures of nkeys seeded keys made by the CPU oracle, message lengths around SHA-512's padding
    boundaries behind the 64-byte R || A prefix, about a fifth corrupted (R or s, one bit).  strict =
    oracle.verify_strict_many; a flipped bit of R or s fails the cofactorless equation too, so the
    un-flipped mask is both expectations (the tests also ask the oracle for a cofactorless sample)."""
    rng = np.random.default_rng(seed)
    seeds = rng.integers(0, 256, (nkeys, 32), dtype=np.uint8)
    pks = [orc.pubkey(s.tobytes()) for s in seeds]
    which = rng.permutation(np.concatenate([np.arange(nkeys), rng.integers(0, nkeys, n - nkeys)]))
    ln = np.array([0, 47, 48, 111, 112, 239, 240, 1000], np.uint64)[rng.integers(0, 8, n)]
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    data = rng.integers(0, 256, int(ln.sum()) + 1, dtype=np.uint8)
    pk = np.frombuffer(b"".join(pks[k] for k in which), np.uint8).reshape(n, 32)
    sig = np.frombuffer(b"".join(orc.sign(seeds[k].tobytes(), pks[k], data[int(o):int(o + l)].tobytes())
                                 for k, o, l in zip(which, off, ln)), np.uint8).reshape(n, 64).copy()
    flip = rng.random(n) < 0.2
    in_r = rng.random(n) < 0.5
    sig[flip & in_r, 7] ^= 0x10
    sig[flip & ~in_r, 40] ^= 0x01
    want = orc.verify_strict_many(pk, sig, data, off, ln, nthreads=8).astype(bool)
    assert np.array_equal(want, ~flip) and 0.15 * n < flip.sum() < 0.25 * n
    return Batch(pk, sig, data, off, ln, want, ~flip)


def with_bad_slices(b, at):
    """b with the message slices of the three items `at` out of bounds (past the end, longer than the buffer,
    off + len wrapping): those items rejected, every other verdict as before"""
    off, ln = b.off.copy(), b.ln.copy()
    size = len(b.msg)
    off[at[0]], ln[at[0]] = size + 1, 0
    off[at[1]], ln[at[1]] = 0, size + 1
    off[at[2]], ln[at[2]] = 2 ** 64 - 8, 16
    strict, cof = b.strict.copy(), b.cofactorless.copy()
    strict[list(at)] = False
    cof[list(at)] = False
    return Batch(b.pk, b.sig, b.msg, off, ln, strict, cof)


class Groups:
    """tests/golden/batch_groups.npz (certificates of 0 .. 67 votes) and the oracle's per-signature bits of its
    630 signatures, computed once; tiled(reps) = the fixture `reps` times over with the tiled expectations"""

    def __init__(self, orc=None, sig_bits=None):
        g = np.load(os.path.join(GOLD, "batch_groups.npz"))
        self.base = {k: g[k] for k in g.files}
        assert int(g["cnt"].max()) == 67 and int(g["cnt"].min()) == 0
        if sig_bits is None:
            og, osb = orc.verify_batch_groups(g["pk"], g["sig"], g["first"], g["cnt"], g["msg32"], nthreads=8)
            assert np.array_equal(og.astype(bool), g["expect"].astype(bool))
            sig_bits = osb
        self.sig_bits = np.asarray(sig_bits).astype(bool)
        self.uniq, inv = np.unique(g["pk"], axis=0, return_inverse=True)
        self.key_idx = inv.ravel().astype(np.uint32)

    def tiled(self, reps):
        g, nsig = self.base, len(self.base["pk"])
        return types.SimpleNamespace(
            n=nsig * reps, pk=np.tile(g["pk"], (reps, 1)), sig=np.tile(g["sig"], (reps, 1)),
            first=np.concatenate([g["first"] + r * nsig for r in range(reps)]).astype(np.uint64),
            cnt=np.tile(g["cnt"], reps).astype(np.uint32), msg32=np.tile(g["msg32"].reshape(-1, 32), (reps, 1)),
            expect=np.tile(g["expect"], reps).astype(bool), sig_bits=np.tile(self.sig_bits, reps),
            key_idx=np.tile(self.key_idx, reps))


class DevBatch:
    """device copies of a Batch, verified through nt_dev_ed25519_verify"""

    def __init__(self, be, b):
        import torch
        self.be, self.torch, self.n = be, torch, b.n
        self.dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(np.array(a, order="C")).to(self.dev)  # a writable copy: fixtures are read-only
        self.pk, self.sig, self.msg = up(b.pk), up(b.sig), up(b.msg)
        self.off, self.ln = up(b.off.view(np.int64)), up(b.ln.view(np.int64))
        torch.cuda.synchronize(self.dev)

    def words(self, mode, stream):
        """the verdict words of one launch, read back once it is done"""
        t = self.torch
        out = t.zeros((self.n + 63) // 64, dtype=t.int64, device=self.dev)
        t.cuda.synchronize(self.dev)  # zeroed on torch's stream, written on the library's
        self.be.dev_verify(0, stream, mode, self.pk.data_ptr(), self.sig.data_ptr(), self.msg.data_ptr(),
                           int(self.msg.numel()), self.off.data_ptr(), self.ln.data_ptr(), self.n, out.data_ptr())
        t.cuda.synchronize(self.dev)
        return out.cpu().numpy().copy()

    def bits(self, mode, stream):
        return np.unpackbits(self.words(mode, stream).view(np.uint8), bitorder="little")[:self.n].astype(bool)


class Counters:
    """deltas of the key-table cache's counters (nt_memory_info | NT_INFO_KTAB) of one context"""
    KEYS = ("used", "fast_rows", "builds", "old_rows")

    def __init__(self, be):
        self.be = be
        self.last = be.ktab_info(0)

    def delta(self):
        now = self.be.ktab_info(0)
        d = {k: now[k] - self.last[k] for k in self.KEYS}
        self.last = now
        return d


def mixed_keyset_case(c, reps, nkeys):
    """The corpus tiled `reps` times for a key set of its distinct keys in mixed mode, unknown key indices and
    strict bits as tests/_keyset_per_lane_probe.py sets them: (key indices, expected verdicts)."""
    uniq, inv = np.unique(c["pk"], axis=0, return_inverse=True)
    assert len(uniq) == nkeys
    idx = np.tile(inv.ravel().astype(np.uint32), reps)
    n = len(idx)
    unknown = (np.arange(n) % 97) == 5
    idx[unknown] = nkeys + 3
    strict = (np.arange(n) % 3) == 1
    midx = (idx | np.where(strict, np.uint32(ntcrypto.NT_KEY_STRICT_BIT), np.uint32(0))).astype(np.uint32)
    want = np.where(strict, np.tile(c["strict"], reps), np.tile(c["batch_rule"], reps)).astype(bool) & ~unknown
    return midx, want
