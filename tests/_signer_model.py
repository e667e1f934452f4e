"""TEST INFRASTRUCTURE: the model of the signer's outputs shared by tests/test_signer_host.py
and tests/test_gpu_signer.py -- tests/_wire.py's Vote signed by the CPU oracle -- and the
edge values both run."""
import numpy as np

import _wire as W


def model_vote(orc, seed, id_, round_, origin):
    """(wire bytes of PrimaryMessage::Vote, Vote::digest) as the reference makes them"""
    pk = orc.pubkey(seed)
    v = W.Vote(id_, round_, origin, pk)
    v.sig = orc.sign(seed, pk, v.digest())
    return W.message(v), v.digest()


def edge_triples(rng, signer_pk):
    """(id, round, origin): ids of all zero / all 0xff bytes, rounds 0, 1, 2^32 and 2^64 - 1,
    the signer as origin, origins that are no curve points"""
    rnd = lambda: rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    # y = 2 has no x on the curve; 0xff.. is not even a canonical field element
    not_points = [bytes([2]) + bytes(31), b"\xff" * 32, bytes(32)]
    out = []
    for id_ in (bytes(32), b"\xff" * 32, rnd()):
        for round_ in (0, 1, 1 << 32, (1 << 64) - 1):
            out.append((id_, round_, rnd()))
    out += [(rnd(), 7, signer_pk), (bytes(32), 0, signer_pk)]
    out += [(rnd(), 3, p) for p in not_points]
    return out
