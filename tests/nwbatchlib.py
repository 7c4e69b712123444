"""Batches for the tests of seqalign_nw_batch's pipeline (sa_batch.hip) and of seqalign_host_legs_nw."""
from __future__ import annotations

import numpy as np

from seqalign_amd import workloads as W


def half_packed_ragged(n: int = 1300, seed: int = 3131, max_len: int = 40):
    """(batch, pairs): n pairs with lengths 0 .. max_len, among them ("", ""), ("A", ""), ("", "C") and runs of ("G", "G").
    The first half lies in the arena as W.from_pairs lays it (a, b, a, b, ...: the host blocks there are `packed`, one copy per
    task); the second half's sequences lie interleaved out of order (every seq_b first, the pairs backwards, then every seq_a), so
    its blocks are packed pair by pair."""
    rng = W.Rng(seed)
    lens = rng.below(max_len + 1, 2 * n).astype(int)
    letters = rng.below(4, int(lens.sum()) + 1).astype(np.int64)
    text = W.DNA[letters].tobytes()
    pairs, at = [], 0
    for k in range(n):
        la, lb = int(lens[2 * k]), int(lens[2 * k + 1])
        a = text[at:at + la]; at += la
        b = (a[:lb] + text[at:at + max(0, lb - la)]) if k % 3 == 0 else text[at:at + lb]   # (every third pair: related sequences)
        at += lb
        pairs.append((a, b))
    for k, edge in ((5, (b"", b"")), (6, (b"A", b"")), (7, (b"", b"C")), (n // 2 + 5, (b"", b"")), (n // 2 + 6, (b"A", b"")),
                    (n // 2 + 7, (b"", b"C")), (n - 1, (b"", b""))):
        pairs[k] = edge
    for k0 in (40, n // 2 - 3, n - 30):          # runs of one tiny shape, one of them across the two halves
        for k in range(k0, k0 + 9):
            pairs[k] = (b"G", b"G")
    half = n // 2
    head = W.from_pairs(pairs[:half])
    base = int(head.arena.nbytes) - 1            # (from_pairs ends its arena with one NUL)
    chunks, off_a, off_b, pos = [], [0] * (n - half), [0] * (n - half), base
    for j in reversed(range(n - half)):
        off_b[j] = pos; chunks.append(pairs[half + j][1]); pos += len(pairs[half + j][1])
    for j in range(n - half):
        off_a[j] = pos; chunks.append(pairs[half + j][0]); pos += len(pairs[half + j][0])
    arena = np.concatenate([head.arena[:base], np.frombuffer(b"".join(chunks) + b"\0", np.uint8)])
    batch = W.Batch(arena,
                    np.concatenate([head.off_a, np.asarray(off_a, np.uint64)]),
                    np.asarray([len(a) for a, _ in pairs], np.uint32),
                    np.concatenate([head.off_b, np.asarray(off_b, np.uint64)]),
                    np.asarray([len(b) for _, b in pairs], np.uint32))
    return batch, pairs


def ragged_related(n: int, lo: int, hi: int, seed: int):
    """n pairs laid out pair by pair, len_a and len_b uniform in lo .. hi, seq_b a 90 % copy of seq_a (alignments with runs)."""
    rng = W.Rng(seed)
    a = W.DNA[rng.below(4, n * hi).astype(np.int64)].reshape(n, hi)
    b = np.where(rng.unit(n * hi).reshape(n, hi) < 0.9, a, W.DNA[rng.below(4, n * hi).astype(np.int64)].reshape(n, hi))
    la = (lo + rng.below(hi - lo + 1, n)).astype(np.int64)
    lb = (lo + rng.below(hi - lo + 1, n)).astype(np.int64)
    cols = np.arange(hi)
    rows = np.concatenate([a, b], axis=1)                                   # pair k's letters in arena order: a's, then b's
    keep = np.concatenate([cols[None, :] < la[:, None], cols[None, :] < lb[:, None]], axis=1)
    arena = np.concatenate([rows[keep], np.zeros(1, np.uint8)])
    ends = np.cumsum(np.stack([la, lb], axis=1).reshape(-1))
    off_a = np.concatenate([[0], ends[1:-1:2]]).astype(np.uint64)
    return W.Batch(arena, off_a, la.astype(np.uint32), off_a + la.astype(np.uint64), lb.astype(np.uint32))
