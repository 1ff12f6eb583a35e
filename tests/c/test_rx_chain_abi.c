/*
 * A plain C caller of the receive verify over fragment chains (rns_rx_verify_chain_dev), bound the
 * way the reference's Rust would bind it (extern "C" + raw pointers): no torch, no Python, the HIP
 * runtime only for device memory.  60 datagrams — IPv4 TCP, IPv6 TCP and IPv4 ICMP, every fifth
 * with a flipped byte — lie in shuffled pool buffers as recv_packet leaves them (512-byte
 * fragments, netif.rs:65-83) or cut at odd places; every status and L4 value is checked against the
 * receive path restated here over the oracle's primitives (oracle/csum_oracle.c, linked as test
 * infrastructure only): header checksum over the first fragment, trim_head, the pseudo-header
 * with the chain's length, compute_buffer_ones_comp over the trimmed fragments.
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

static uint64_t rng_state = 0x5C4A1Full;
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

enum { N = 60, BUF = 512, MAXLEN = 2048, MAXFR = 8, NBUF = N * MAXFR };

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

/* The receive path over the chain (fragments fo/fl of pool), first fragment >= the IP header. */
static void reference(const uint8_t *pool, const uint64_t *fo, const uint32_t *fl, uint32_t nf, uint8_t *status,
                      uint16_t *l4)
{
    const uint8_t *header = pool + fo[0];
    const int v6 = (header[0] >> 4) == 6;
    const uint32_t hdr = v6 ? 40 : (header[0] & 0xfu) * 4u;
    uint32_t total = 0;
    for (uint32_t f = 0; f < nf; ++f)
        total += fl[f];
    uint8_t st = (v6 || oracle_compute_checksum(header, hdr) == 0) ? RNS_RX_IP_OK : 0;
    const uint8_t proto = v6 ? header[6] : header[9];
    const uint8_t *base[MAXFR];
    size_t len[MAXFR];
    size_t k = 0;
    for (uint32_t f = 0; f < nf; ++f) {  /* trim_head(hdr): the head fragment holds the header */
        const uint32_t cut = f == 0 ? hdr : 0;
        if (fl[f] > cut) {
            base[k] = pool + fo[f] + cut;
            len[k++] = fl[f] - cut;
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
    static uint8_t pool[NBUF * BUF + 16], dgram[MAXFR * BUF], status[N], ref_status[N];
    static uint16_t l4[N], ref_l4[N];
    static uint64_t off[NBUF];
    static uint32_t len[NBUF], first[N + 1], order[NBUF];
    for (uint32_t j = 0; j < NBUF; ++j)
        order[j] = j;
    for (uint32_t j = NBUF - 1; j > 0; --j) {  /* a pool whose buffers have been in use: any order */
        const uint32_t r = (uint32_t)(next_u64() % (j + 1)), t = order[j];
        order[j] = order[r];
        order[r] = t;
    }
    memset(pool, 0xEE, sizeof pool);
    uint32_t nf = 0;
    int accepted = 0;
    for (uint32_t i = 0; i < N; ++i) {
        const int k = (int)(i % 3);
        const uint32_t hdr = k == 1 ? 40 : 20;
        /* fragment lengths first: i even, a datagram cut into full buffers as recv_packet leaves it;
         * i odd, cut at odd places (the first fragment holds the header and 1 or 3 bytes more) */
        uint32_t fl[MAXFR], nfr = 0, dl = 0;
        if (i & 1) {
            nfr = 2 + (uint32_t)(next_u64() % (MAXFR - 1));
            fl[0] = hdr + 1 + (i & 2);
            fl[1] = 20 + (uint32_t)(next_u64() % (BUF - 22));
            for (uint32_t f = 2; f < nfr; ++f)
                fl[f] = 1 + (uint32_t)(next_u64() % (BUF - 2));
            for (uint32_t f = 0; f < nfr; ++f)
                dl += fl[f];
        } else {
            dl = hdr + 20 + (uint32_t)(next_u64() % (MAXLEN - hdr - 20 + 1));
            for (uint32_t pos = 0; pos < dl; pos += BUF)
                fl[nfr++] = dl - pos < BUF ? dl - pos : BUF;
        }
        make_datagram(dgram, dl, k);
        if (i % 5 == 4)
            dgram[hdr + (next_u64() % (dl - hdr))] ^= 0x10;
        first[i] = nf;
        for (uint32_t f = 0, pos = 0; f < nfr; pos += fl[f++]) {
            off[nf] = (uint64_t)order[nf] * BUF + ((i & 1) ? (uint32_t)(next_u64() % 3) : 0);  /* odd: <= BUF - 2 bytes */
            len[nf] = fl[f];
            memcpy(pool + off[nf], dgram + pos, fl[f]);
            ++nf;
        }
        reference(pool, off + first[i], len + first[i], nf - first[i], &ref_status[i], &ref_l4[i]);
        accepted += (ref_status[i] & RNS_RX_ACCEPT) != 0;
    }
    first[N] = nf;
    /* the intact full-buffer chains verify; a chain cut at odd places folds differently (util.rs:97-99) */
    CHECK(accepted >= N / 3 && accepted <= N / 2, "the oracle accepts %d of %d", accepted, N);

    /* argument checks need no device */
    CHECK(rns_rx_verify_chain_dev(NULL, 0, NULL, NULL, 0, NULL, 0, NULL, NULL, NULL, NULL, NULL) == RNS_OK, "n == 0");
    CHECK(rns_rx_verify_chain_dev(pool, sizeof pool, off, len, nf, first, N, local4, local6, NULL, NULL, NULL) ==
              RNS_E_INVALID, "NULL status");
    CHECK(rns_rx_verify_chain_dev(pool, sizeof pool, NULL, len, nf, first, N, local4, local6, status, NULL, NULL) ==
              RNS_E_INVALID, "NULL offsets");

    uint8_t *d_pool = NULL, *d_status = NULL;
    uint16_t *d_l4 = NULL;
    uint64_t *d_off = NULL;
    uint32_t *d_len = NULL, *d_first = NULL;
    hipStream_t st;
    if (hipMalloc((void **)&d_pool, sizeof pool) != hipSuccess) {
        fprintf(stderr, "hipMalloc failed: no usable device\n");
        return 2;
    }
    HIP_OK(hipMalloc((void **)&d_status, N));
    HIP_OK(hipMalloc((void **)&d_l4, N * sizeof *l4));
    HIP_OK(hipMalloc((void **)&d_off, NBUF * sizeof *off));
    HIP_OK(hipMalloc((void **)&d_len, NBUF * sizeof *len));
    HIP_OK(hipMalloc((void **)&d_first, (N + 1) * sizeof *first));
    HIP_OK(hipStreamCreate(&st));
    HIP_OK(hipMemcpy(d_pool, pool, sizeof pool, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_off, off, NBUF * sizeof *off, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_len, len, NBUF * sizeof *len, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_first, first, (N + 1) * sizeof *first, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_status, 0x55, N));
    CHECK(rns_rx_verify_chain_dev(d_pool, sizeof pool, d_off, d_len, nf, d_first, N, local4, local6, d_status, d_l4, st) ==
              RNS_OK, "rns_rx_verify_chain_dev");
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipMemcpy(status, d_status, N, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(l4, d_l4, N * sizeof *l4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < N; ++i) {
        CHECK(status[i] == ref_status[i], "status %u: %02x != %02x", i, status[i], ref_status[i]);
        CHECK(l4[i] == ref_l4[i], "l4 %u: %04x != %04x", i, l4[i], ref_l4[i]);
    }
    /* without the L4 array; the pool is only read */
    HIP_OK(hipMemset(d_status, 0x55, N));
    CHECK(rns_rx_verify_chain_dev(d_pool, sizeof pool, d_off, d_len, nf, d_first, N, local4, local6, d_status, NULL, st) ==
              RNS_OK, "no L4 array");
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipMemcpy(status, d_status, N, hipMemcpyDeviceToHost));
    CHECK(memcmp(status, ref_status, N) == 0, "without the L4 array: statuses differ");
    static uint8_t back[sizeof pool];
    HIP_OK(hipMemcpy(back, d_pool, sizeof pool, hipMemcpyDeviceToHost));
    CHECK(memcmp(back, pool, sizeof pool) == 0, "the pool changed");
    hipStreamDestroy(st);
    hipFree(d_pool); hipFree(d_status); hipFree(d_l4); hipFree(d_off); hipFree(d_len); hipFree(d_first);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
