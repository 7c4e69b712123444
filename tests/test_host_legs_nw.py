"""seqalign_host_legs_nw (sa_batch.hip): the host legs of seqalign_nw_batch's moves form with no device involved -- sizes, offsets
and packing by the loops the call itself runs, then the expansion of synthetic all-MATCH moves.  The outputs show the expansion
leg only (it reads the caller's arena): that the offsets and packing passes are right is seen through seqalign_nw_batch's GPU tests.
No GPU needed."""
from __future__ import annotations

import ctypes as C
import hashlib

import numpy as np

import nwbatchlib as NB
import seqalign_amd as S

# what the library gave for this batch before the packing and offsets loops became shared functions (sha256 over out_len and over
# every pair's two strings in pair order; the lengths' sum; pairs 0, 3 and 700)
WANT_SHA = "956a0b39f3adddd45d970f85885634dd24f835137b04c82f5fa2db9d3a01bb62"
WANT_LEN_SUM = 33321
WANT_SAMPLES = {0: (5, b"CCCAT", b"---CC"),
                3: (36, b"AGACCCATCGGGTCAAAGGGTCTCTATTAATCTGGA", b"---AGACCCATCGGGTCAAAGGGTCTCTATTAATCT"),
                700: (25, b"--CCGTGGGGAGCGATCGGTACTCC", b"CGATACCCGGACCCACACTCACATA")}


def run_host_legs(batch, iterations=2):
    n = batch.n_pairs
    caps = batch.len_a.astype(np.uint64) + batch.len_b.astype(np.uint64) + np.uint64(1)
    str_off = np.zeros(n, np.uint64)
    str_off[1:] = np.cumsum(caps)[:-1]
    total = int(caps.sum()) + 1
    out_a, out_b = np.full(total, 0x7E, np.uint8), np.full(total, 0x7E, np.uint8)
    out_len = np.full(n, 0xFFFFFFFF, np.uint32)
    pack, expand = C.c_double(-1), C.c_double(-1)
    d = S.batch_desc(batch)
    rc = S.lib().seqalign_host_legs_nw(C.byref(d), S._ptr(str_off), S._ptr(out_a), S._ptr(out_b), S._ptr(out_len),
                                       C.c_int(iterations), C.byref(pack), C.byref(expand))
    strings = [(out_a[int(o):int(o) + int(ln)].tobytes(), out_b[int(o):int(o) + int(ln)].tobytes()) for o, ln in zip(str_off, out_len)]
    return rc, out_len, strings, pack.value, expand.value


def test_host_legs_nw_on_packed_and_unpacked_blocks():
    batch, pairs = NB.half_packed_ragged()
    assert batch.n_pairs == 1300 and [(batch.seq_a(p), batch.seq_b(p)) for p in range(1300)] == pairs
    rc, out_len, strings, pack_ms, expand_ms = run_host_legs(batch)
    assert rc == 0 and pack_ms >= 0 and expand_ms >= 0
    h = hashlib.sha256(out_len.tobytes())
    for sa, sb in strings:
        h.update(sa); h.update(b"|"); h.update(sb); h.update(b"\n")
    print("host legs:", h.hexdigest(), int(out_len.sum()), {p: (int(out_len[p]), *strings[p]) for p in (0, 3, 700)})
    assert int(out_len.sum()) == WANT_LEN_SUM
    for p, want in WANT_SAMPLES.items():
        assert (int(out_len[p]), *strings[p]) == want, p
    assert h.hexdigest() == WANT_SHA

