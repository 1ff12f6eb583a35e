"""Helpers of the pool transmit tests (rns_tx_fill_pool_dev, rns_io_send_batch_pool): datagrams cut
into [head, payload] laid into a pool of fixed-size buffers as the reference's transmit path leaves
them (alloc_header's head at its buffer's end, buf.rs:262-291; append_from_slice's payload in whole
buffers and a last partly filled one, buf.rs:385-420), and the CSR chains the compact form means."""
import numpy as np

from oracle import oracle as O
from rustnetworkstack_amd.batch import tx_pool_layout


def lay_pool(heads, pays, buf, shuffled=True, seed=1, spare=3):
    """(pool uint8, buf_idx uint32, blk_first uint32, head_len8 uint8, pay_len16 uint16, first):
    buffers in order or a seeded permutation, `spare` unused ones among them, every byte the
    datagrams do not use random."""
    hl = np.array([len(h) for h in heads], dtype=np.uint8)
    pl = np.array([len(p) for p in pays], dtype=np.uint16)
    blk, first, nf = tx_pool_layout(pl, buf)
    nbuf = nf + spare
    order = np.random.default_rng(seed).permutation(nbuf) if shuffled else np.arange(nbuf)
    idx = order[:nf].astype(np.uint32)
    pool = np.frombuffer(O.splitmix64_bytes(seed ^ 0x7001, nbuf * buf).tobytes(), dtype=np.uint8).copy()
    place(pool.reshape(nbuf, buf), idx, first, heads, pays, buf)
    return pool, idx, blk, hl, pl, first


def place(rows, idx, first, heads, pays, buf):
    """Write the datagrams into the buffers idx names (rows = the pool, or any [k, buf] array with
    idx indexing its rows)."""
    for i, (h, p) in enumerate(zip(heads, pays)):
        f0 = int(first[i])
        if h:
            rows[idx[f0], buf - len(h):] = np.frombuffer(h, dtype=np.uint8)
        for j in range(0, len(p), buf):
            piece = p[j:j + buf]
            rows[idx[f0 + 1 + j // buf], :len(piece)] = np.frombuffer(piece, dtype=np.uint8)


def expand(idx, blk_first, hl, pl, buf, n_frags=None):
    """The CSR chains the compact form means (rns_checksum.h): (frag_off uint64, frag_len uint32,
    first uint32).  A datagram whose range runs past n_frags gets no fragments (both forms call it
    malformed)."""
    n_frags = idx.size if n_frags is None else n_frags
    n = pl.size
    nfr = 1 + -(-pl.astype(np.int64) // buf)
    f0 = np.zeros(n, dtype=np.int64)
    for b in range(0, n, 64):
        c = np.cumsum(nfr[b:b + 64])
        f0[b:b + 64] = int(blk_first[b // 64]) + c - nfr[b:b + 64]
    ok = f0 + nfr <= n_frags
    cnt = np.where(ok, nfr, 0)
    first = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(cnt, out=first[1:])
    nf = int(first[-1])
    owner = np.repeat(np.arange(n), cnt)
    k = np.arange(nf) - first[owner]                       # fragment number within its datagram
    off = idx.astype(np.uint64)[f0[owner] + k] * np.uint64(buf)
    ln = np.full(nf, buf, dtype=np.int64)
    last = (k == cnt[owner] - 1) & (k > 0)
    ln[last] = (pl.astype(np.int64)[owner] - (k - 1) * buf)[last]
    head = k == 0
    ln[head] = hl.astype(np.int64)[owner][head]
    off[head] += (buf - hl.astype(np.int64)[owner][head]).astype(np.uint64)
    return off, ln.astype(np.uint32), first.astype(np.uint32)


def mask_slack(pool, ref, free, blk_first, head_len8, pay_len16, B):
    """The bytes a builder into the transmit form may leave unspecified — from a payload's end to the next
    16-byte boundary of its last buffer — copied from ref into pool."""
    from icmp_echo_helper import expand_replies
    for fr, hl in zip(expand_replies(free, blk_first, head_len8, pay_len16, B), head_len8):
        if hl and len(fr) > 1 and fr[-1][2] % 16:
            k, _, e = fr[-1]
            pool[k * B + e:k * B + ((e + 15) & ~15)] = ref[k * B + e:k * B + ((e + 15) & ~15)]
