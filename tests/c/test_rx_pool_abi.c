/*
 * A plain C caller of the receive verify over pool buffers (rns_rx_verify_pool_dev) and its host
 * layout helper (rns_rx_pool_layout), bound the way the reference's Rust would bind them (extern "C"
 * + raw pointers): no torch, no Python, the HIP runtime only for device memory.  150 datagrams —
 * IPv4 TCP, IPv6 TCP and IPv4 ICMP, every fifth with a flipped byte, one of them empty — lie in
 * shuffled 512-byte pool buffers as recv_packet leaves them (netif.rs:65-83).  Every status and L4
 * value is checked against the receive path restated here over the oracle's primitives
 * (oracle/csum_oracle.c, linked as test infrastructure only) and against rns_rx_verify_chain_dev on
 * the CSR chains the compact form expands to.
 *
 * Prints "all checks passed" and exits 0 on success; exits 2 when no device memory can be had.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rns_checksum.h"

int32_t oracle_compute_ones_comp(uint16_t in_checksum, const uint8_t *slice, size_t len);
int32_t oracle_compute_checksum(const uint8_t *slice, size_t len);
int32_t oracle_compute_buffer_ones_comp(uint16_t initial_sum, const uint8_t *const *frag_base, const size_t *frag_len,
                                        size_t nfrags);
int32_t oracle_compute_pseudo_header_checksum(const uint8_t *src, size_t src_len, const uint8_t *dst, size_t dst_len,
                                              uint64_t length, uint8_t protocol);

static uint64_t rng_state = 0x9001F00Dull;
static uint64_t next_u64(void)
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int failures = 0;
#define CHECK(cond, ...)                                                                           \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            if (failures++ < 10) {                                                                 \
                fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);                               \
                fprintf(stderr, __VA_ARGS__);                                                      \
                fprintf(stderr, "\n");                                                             \
            }                                                                                      \
        }                                                                                          \
    } while (0)
#define HIP_OK(x)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_));              \
            return 2;                                                                              \
        }                                                                                          \
    } while (0)

enum { N = 150, LOG2 = 9, BUF = 1 << LOG2, MAXLEN = 2048, MAXFR = MAXLEN / BUF, NBUF = N * MAXFR, NBLK = (N + 63) / 64,
       EMPTY = 77 };

static const uint8_t local4[4] = {10, 0, 0, 2}, remote4[4] = {10, 0, 0, 1};
static uint8_t local6[16], remote6[16];

/* A valid datagram of kind k (0: IPv4 TCP, 1: IPv6 TCP, 2: IPv4 ICMP) and `len` bytes in p. */
static void make_datagram(uint8_t *p, uint32_t len, int k)
{
    const uint32_t hdr = k == 1 ? 40 : 20;
    for (uint32_t b = 0; b < len; ++b)
        p[b] = (uint8_t)next_u64();
    memset(p, 0, hdr);
    uint8_t *seg = p + hdr;
    const uint32_t sl = len - hdr;
    if (k == 1) {
        p[0] = 0x60; p[4] = (uint8_t)(sl >> 8); p[5] = (uint8_t)sl; p[6] = 6; p[7] = 64;
        memcpy(p + 8, remote6, 16);
        memcpy(p + 24, local6, 16);
    } else {
        p[0] = 0x45; p[2] = (uint8_t)(len >> 8); p[3] = (uint8_t)len; p[6] = 0x40; p[8] = 64; p[9] = k == 0 ? 6 : 1;
        memcpy(p + 12, remote4, 4);
        memcpy(p + 16, local4, 4);
        const uint16_t c = (uint16_t)oracle_compute_checksum(p, 20);
        p[10] = (uint8_t)(c >> 8); p[11] = (uint8_t)c;
    }
    const uint32_t field = k == 2 ? 2 : 16;
    seg[field] = seg[field + 1] = 0;
    const uint16_t ph = k == 2 ? 0
        : (uint16_t)oracle_compute_pseudo_header_checksum(k == 1 ? remote6 : remote4, k == 1 ? 16 : 4,
                                                          k == 1 ? local6 : local4, k == 1 ? 16 : 4, sl, 6);
    const uint16_t c = (uint16_t)(0xffff ^ oracle_compute_ones_comp(ph, seg, sl));
    seg[field] = (uint8_t)(c >> 8); seg[field + 1] = (uint8_t)c;
}

/* The receive path over a datagram of `total` bytes in the buffers idx[0..): the header from the
 * first buffer, trim_head, compute_buffer_ones_comp over the trimmed fragments. */
static void reference(const uint8_t *pool, const uint32_t *idx, uint32_t total, uint8_t *status, uint16_t *l4)
{
    *l4 = 0;
    *status = RNS_RX_MALFORMED;
    if (total == 0)  /* no fragments: header() asserts */
        return;
    const uint8_t *header = pool + (uint64_t)idx[0] * BUF;
    const int v6 = (header[0] >> 4) == 6;
    const uint32_t hdr = v6 ? 40 : (header[0] & 0xfu) * 4u;
    uint8_t st = (v6 || oracle_compute_checksum(header, hdr) == 0) ? RNS_RX_IP_OK : 0;
    const uint8_t proto = v6 ? header[6] : header[9];
    const uint8_t *base[MAXFR];
    size_t len[MAXFR];
    size_t k = 0;
    for (uint32_t f = 0, pos = 0; pos < total; ++f, pos += BUF) {
        const uint32_t fl = total - pos < BUF ? total - pos : BUF, cut = f == 0 ? hdr : 0;
        if (fl > cut) {
            base[k] = pool + (uint64_t)idx[f] * BUF + cut;
            len[k++] = fl - cut;
        }
    }
    const uint16_t ph = proto == 1 ? 0
        : (uint16_t)oracle_compute_pseudo_header_checksum(header + (v6 ? 8 : 12), v6 ? 16 : 4, v6 ? local6 : local4,
                                                          v6 ? 16 : 4, total - hdr, proto);
    *l4 = (uint16_t)(0xffff ^ (k ? oracle_compute_buffer_ones_comp(ph, base, len, k) : ph));
    if (*l4 == 0)
        st |= RNS_RX_L4_OK;
    if ((st & RNS_RX_IP_OK) && (st & RNS_RX_L4_OK))
        st |= RNS_RX_ACCEPT;
    *status = st;
}

int main(void)
{
    for (int b = 0; b < 16; ++b) {
        local6[b] = (uint8_t)(b == 0 ? 0xfd : b == 15 ? 2 : 0);
        remote6[b] = (uint8_t)(b == 0 ? 0xfd : b == 15 ? 1 : 0);
    }
    static uint8_t pool[NBUF * BUF], dgram[MAXLEN], status[N], chain_status[N], ref_status[N];
    static uint16_t len16[N], l4[N], chain_l4[N], ref_l4[N];
    static uint32_t idx[NBUF], blk_first[NBLK], first[N + 1], frag_len[NBUF], order[NBUF];
    static uint64_t frag_off[NBUF];
    for (uint32_t j = 0; j < NBUF; ++j)
        order[j] = j;
    for (uint32_t j = NBUF - 1; j > 0; --j) {  /* a pool whose buffers have been in use: any order */
        const uint32_t r = (uint32_t)(next_u64() % (j + 1)), t = order[j];
        order[j] = order[r];
        order[r] = t;
    }
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t hdr = i % 3 == 1 ? 40 : 20;
        const uint32_t edge[] = {BUF - 1, BUF, BUF + 1, 2 * BUF, 2 * BUF + 1, MAXLEN, hdr + 20};
        len16[i] = (uint16_t)(i == EMPTY ? 0 : i < 7 ? edge[i] : hdr + 20 + next_u64() % (MAXLEN - hdr - 20 + 1));
    }

    /* the layout helper: the index of the compact form and of the chains it expands to */
    uint64_t nf64 = 0;
    CHECK(rns_rx_pool_layout(len16, N, 5, blk_first, first, &nf64) == RNS_E_INVALID, "buf_log2 5");
    CHECK(rns_rx_pool_layout(len16, N, LOG2, blk_first, first, NULL) == RNS_E_INVALID, "NULL n_frags");
    CHECK(rns_rx_pool_layout(len16, N, LOG2, blk_first, first, &nf64) == RNS_OK, "layout");
    const uint32_t nf = (uint32_t)nf64;
    CHECK(first[0] == 0 && first[N] == nf && nf <= NBUF, "first[0], first[N] = %u, %u", first[0], first[N]);
    for (uint32_t i = 0; i < N; ++i) {
        CHECK(first[i + 1] - first[i] == (len16[i] + BUF - 1u) / BUF, "fragments of datagram %u", i);
        CHECK((i & 63) || blk_first[i >> 6] == first[i], "blk_first[%u]", i >> 6);
    }

    memset(pool, 0xEE, sizeof pool);
    int accepted = 0;
    for (uint32_t i = 0; i < N; ++i) {
        const int k = (int)(i % 3);
        const uint32_t hdr = k == 1 ? 40 : 20, dl = len16[i];
        if (dl) {
            make_datagram(dgram, dl, k);
            if (i % 5 == 4)
                dgram[hdr + (next_u64() % (dl - hdr))] ^= 0x10;
        }
        for (uint32_t f = first[i], pos = 0; f < first[i + 1]; ++f, pos += BUF) {
            idx[f] = order[f];
            frag_off[f] = (uint64_t)idx[f] << LOG2;
            frag_len[f] = dl - pos < BUF ? dl - pos : BUF;
            memcpy(pool + frag_off[f], dgram + pos, frag_len[f]);
        }
        reference(pool, idx + first[i], dl, &ref_status[i], &ref_l4[i]);
        accepted += (ref_status[i] & RNS_RX_ACCEPT) != 0;
    }
    CHECK(accepted == N - N / 5 - 1, "the oracle accepts %d of %d", accepted, N);
    CHECK(ref_status[EMPTY] == RNS_RX_MALFORMED, "the empty datagram");

    /* argument checks need no device */
    CHECK(rns_rx_verify_pool_dev(NULL, 0, 0, NULL, 0, NULL, NULL, 0, NULL, NULL, NULL, NULL, NULL) == RNS_OK, "n == 0");
    CHECK(rns_rx_verify_pool_dev(pool, sizeof pool, LOG2, idx, nf, blk_first, len16, N, local4, local6, NULL, NULL, NULL) ==
              RNS_E_INVALID, "NULL status");
    CHECK(rns_rx_verify_pool_dev(pool, sizeof pool, 16, idx, nf, blk_first, len16, N, local4, local6, status, NULL, NULL) ==
              RNS_E_INVALID, "buf_log2 16");
    CHECK(rns_rx_verify_pool_dev(pool, sizeof pool, LOG2, NULL, nf, blk_first, len16, N, local4, local6, status, NULL,
                                 NULL) == RNS_E_INVALID, "NULL indices");

    uint8_t *d_pool = NULL, *d_status = NULL;
    uint16_t *d_l4 = NULL, *d_len16 = NULL;
    uint64_t *d_off = NULL;
    uint32_t *d_idx = NULL, *d_blk = NULL, *d_len = NULL, *d_first = NULL;
    hipStream_t st;
    if (hipMalloc((void **)&d_pool, sizeof pool) != hipSuccess) {
        fprintf(stderr, "hipMalloc failed: no usable device\n");
        return 2;
    }
    HIP_OK(hipMalloc((void **)&d_status, N));
    HIP_OK(hipMalloc((void **)&d_l4, N * sizeof *l4));
    HIP_OK(hipMalloc((void **)&d_len16, N * sizeof *len16));
    HIP_OK(hipMalloc((void **)&d_idx, NBUF * sizeof *idx));
    HIP_OK(hipMalloc((void **)&d_blk, NBLK * sizeof *blk_first));
    HIP_OK(hipMalloc((void **)&d_off, NBUF * sizeof *frag_off));
    HIP_OK(hipMalloc((void **)&d_len, NBUF * sizeof *frag_len));
    HIP_OK(hipMalloc((void **)&d_first, (N + 1) * sizeof *first));
    HIP_OK(hipStreamCreate(&st));
    HIP_OK(hipMemcpy(d_pool, pool, sizeof pool, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_len16, len16, N * sizeof *len16, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_idx, idx, NBUF * sizeof *idx, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_blk, blk_first, NBLK * sizeof *blk_first, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_off, frag_off, NBUF * sizeof *frag_off, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_len, frag_len, NBUF * sizeof *frag_len, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_first, first, (N + 1) * sizeof *first, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_status, 0x55, N));
    CHECK(rns_rx_verify_pool_dev(d_pool, sizeof pool, LOG2, d_idx, nf, d_blk, d_len16, N, local4, local6, d_status, d_l4,
                                 st) == RNS_OK, "rns_rx_verify_pool_dev");
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipMemcpy(status, d_status, N, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(l4, d_l4, N * sizeof *l4, hipMemcpyDeviceToHost));
    /* the existing entry on the expanded chains, over the same pool */
    HIP_OK(hipMemset(d_status, 0x55, N));
    CHECK(rns_rx_verify_chain_dev(d_pool, sizeof pool, d_off, d_len, nf, d_first, N, local4, local6, d_status, d_l4, st) ==
              RNS_OK, "rns_rx_verify_chain_dev");
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipMemcpy(chain_status, d_status, N, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(chain_l4, d_l4, N * sizeof *l4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < N; ++i) {
        CHECK(status[i] == ref_status[i], "status %u: %02x != %02x", i, status[i], ref_status[i]);
        CHECK(l4[i] == ref_l4[i], "l4 %u: %04x != %04x", i, l4[i], ref_l4[i]);
        CHECK(status[i] == chain_status[i], "status %u: %02x, the chain entry %02x", i, status[i], chain_status[i]);
        CHECK(l4[i] == chain_l4[i], "l4 %u: %04x, the chain entry %04x", i, l4[i], chain_l4[i]);
    }
    /* without the L4 array; the pool is only read */
    HIP_OK(hipMemset(d_status, 0x55, N));
    CHECK(rns_rx_verify_pool_dev(d_pool, sizeof pool, LOG2, d_idx, nf, d_blk, d_len16, N, local4, local6, d_status, NULL,
                                 st) == RNS_OK, "no L4 array");
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipMemcpy(status, d_status, N, hipMemcpyDeviceToHost));
    CHECK(memcmp(status, ref_status, N) == 0, "without the L4 array: statuses differ");
    static uint8_t back[sizeof pool];
    HIP_OK(hipMemcpy(back, d_pool, sizeof pool, hipMemcpyDeviceToHost));
    CHECK(memcmp(back, pool, sizeof pool) == 0, "the pool changed");
    hipStreamDestroy(st);
    hipFree(d_pool); hipFree(d_status); hipFree(d_l4); hipFree(d_len16); hipFree(d_idx); hipFree(d_blk);
    hipFree(d_off); hipFree(d_len); hipFree(d_first);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
