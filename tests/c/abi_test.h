/*
 * The one harness of the plain C callers of the C ABI (tests/c/test_*_abi.c): the random numbers, the
 * checks, the device buffers with their one no-device exit and one ending, big-endian accessors, and
 * the datagram builders and the receive reference that more than one program needs, restated over the
 * oracle's primitives (oracle/csum_oracle.c, linked as test infrastructure only).  Header-only and
 * all `static inline`, so a program is one gcc line and an unused helper is no warning.
 *
 * A program sets its seed first:   #define ABI_TEST_SEED 0x...ull
 *                                  #include "abi_test.h"
 * and ends with                    return abi_finish("%u datagrams", n);
 * which prints "all checks passed (...)" and returns 0, or the number of failed checks and 1.  With no
 * usable device the program exits 2 at its first allocation, or 1 if a check had failed before it.
 */
#ifndef ABI_TEST_H
#define ABI_TEST_H

#include <hip/hip_runtime_api.h>
#include <stdarg.h>
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
void oracle_chain_batch(const uint8_t *arena, const uint64_t *frag_off, const uint32_t *frag_len, const uint32_t *first,
                        const uint16_t *seed, uint16_t *out, size_t npkts, int complement);
void oracle_tx_chain_fill(uint8_t *arena, uint64_t arena_bytes, const uint64_t *frag_off, const uint32_t *frag_len,
                          const uint32_t *first, uint32_t n_frags, size_t n, uint8_t *status);

/* ---- random numbers: splitmix64 from the program's seed ---- */
static uint64_t rng_state = ABI_TEST_SEED;
static inline uint64_t next_u64(void)
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

/* one draw per 8 bytes */
static inline void fill_random(uint8_t *p, uint64_t bytes)
{
    for (uint64_t b = 0; b < bytes; b += 8) {
        const uint64_t w = next_u64();
        memcpy(p + b, &w, bytes - b < 8 ? bytes - b : 8);
    }
}

/* one draw per byte */
static inline void fill_random_bytes(uint8_t *p, size_t bytes)
{
    for (size_t b = 0; b < bytes; ++b)
        p[b] = (uint8_t)next_u64();
}

/* 0..n-1 in any order (a pool whose buffers have been in use): one draw per element but the first */
static inline void shuffled_order(uint32_t *order, uint32_t n)
{
    for (uint32_t j = 0; j < n; ++j)
        order[j] = j;
    for (uint32_t j = n - 1; j > 0; --j) {
        const uint32_t r = (uint32_t)(next_u64() % (j + 1)), t = order[j];
        order[j] = order[r];
        order[r] = t;
    }
}

/* ---- checks: the first ten failures are printed, all are counted, and so are the evaluations ---- */
static int failures = 0;
static unsigned long abi_checks = 0;
#define CHECK(cond, ...)                                                                           \
    do {                                                                                           \
        ++abi_checks;                                                                              \
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

/* ---- device buffers: every allocation is registered, abi_finish() frees them ---- */
enum { ABI_MAX_BUFS = 64 };
static void *abi_bufs[ABI_MAX_BUFS];
static int abi_nbufs = 0, abi_has_stream = 0;
static hipStream_t abi_the_stream;

/* The one no-device exit: 1 if a check has failed without the device, else 2. */
static inline void abi_no_device(void)
{
    if (failures) {
        fprintf(stderr, "%d checks failed before the device was touched\n", failures);
        exit(1);
    }
    fprintf(stderr, "no usable device (%lu checks passed without one)\n", abi_checks);
    exit(2);
}

/* Allocates *d unless it is allocated already (a pointer starts NULL), so UP and OUT also refresh. */
static inline hipError_t abi_alloc(void **d, size_t bytes)
{
    if (*d)
        return hipSuccess;
    const hipError_t e = abi_nbufs < ABI_MAX_BUFS ? hipMalloc(d, bytes) : hipErrorOutOfMemory;
    if (e != hipSuccess && abi_nbufs == 0)
        abi_no_device();
    if (e == hipSuccess)
        abi_bufs[abi_nbufs++] = *d;
    return e;
}
static inline hipError_t abi_up(void **d, const void *host, size_t bytes)
{
    const hipError_t e = abi_alloc(d, bytes);
    return e != hipSuccess ? e : hipMemcpy(*d, host, bytes, hipMemcpyHostToDevice);
}
static inline hipError_t abi_out(void **d, size_t bytes, int fill)
{
    const hipError_t e = abi_alloc(d, bytes);
    return e != hipSuccess ? e : hipMemset(*d, fill, bytes);
}
static inline hipError_t abi_stream(hipStream_t *st)
{
    const hipError_t e = hipStreamCreate(&abi_the_stream);
    abi_has_stream = e == hipSuccess;
    *st = abi_the_stream;
    return e;
}
/* allocate (the first time) and upload / allocate (the first time) and fill with a sentinel / download */
#define UP(d, host, bytes) HIP_OK(abi_up((void **)&(d), (host), (bytes)))
#define OUT(d, bytes, fill) HIP_OK(abi_out((void **)&(d), (bytes), (fill)))
#define DOWN(host, d, bytes) HIP_OK(hipMemcpy((host), (d), (bytes), hipMemcpyDeviceToHost))

/* The one ending: `return abi_finish("%u datagrams", n);` */
__attribute__((format(printf, 1, 2))) static inline int abi_finish(const char *detail, ...)
{
    while (abi_nbufs)
        hipFree(abi_bufs[--abi_nbufs]);
    if (abi_has_stream)
        hipStreamDestroy(abi_the_stream);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    va_list ap;
    va_start(ap, detail);
    printf("all checks passed (%lu checks; ", abi_checks);
    vprintf(detail, ap);
    printf(")\n");
    va_end(ap);
    return 0;
}

/* ---- big-endian accessors ---- */
static inline void put16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 8); p[1] = (uint8_t)v; }
static inline void put32(uint8_t *p, uint32_t v) { put16(p, v >> 16); put16(p + 2, v); }
static inline uint32_t get16(const uint8_t *p) { return (uint32_t)p[0] << 8 | p[1]; }
static inline uint32_t get32(const uint8_t *p) { return get16(p) << 16 | get16(p + 2); }

/* a > b in sequence space (util.rs:155-158) */
static inline int seq_gt(uint32_t a, uint32_t b)
{
    const uint32_t d = a - b;
    return d < 0x80000000u && d != 0;
}

/* ---- datagram builders ---- */
/* The fields of an option-less IPv4 header that ip_output sets before the checksum (DF, TTL 64);
 * the id and the checksum field keep what they hold. */
static inline void ipv4_fields(uint8_t *h, uint32_t total, uint8_t proto, const uint8_t *src, const uint8_t *dst)
{
    h[0] = 0x45; h[1] = 0; put16(h + 2, total); h[6] = 0x40; h[7] = 0; h[8] = 64; h[9] = proto;
    memcpy(h + 12, src, 4);
    memcpy(h + 16, dst, 4);
}
/* The header checksum over the header with its field zeroed, stored (ip.rs:158-159). */
static inline void ipv4_checksum(uint8_t *h, uint32_t hdr)
{
    put16(h + 10, 0);
    put16(h + 10, (uint32_t)oracle_compute_checksum(h, hdr));
}
/* Finishes an IPv4 header of `hdr` bytes whose other fields are set: total length, addresses, checksum. */
static inline void ipv4_finish(uint8_t *h, uint32_t hdr, uint32_t total, const uint8_t *src, const uint8_t *dst)
{
    put16(h + 2, total);
    memcpy(h + 12, src, 4);
    memcpy(h + 16, dst, 4);
    ipv4_checksum(h, hdr);
}
/* An IPv6 header over 40 zeroed bytes: hop limit 64. */
static inline void ipv6_header(uint8_t *h, uint32_t payload, uint8_t next, const uint8_t *src, const uint8_t *dst)
{
    h[0] = 0x60; put16(h + 4, payload); h[6] = next; h[7] = 64;
    memcpy(h + 8, src, 16);
    memcpy(h + 24, dst, 16);
}
/* The L4 checksum of the `sl` bytes at seg, its field zeroed, over the pseudo-header of the two
 * addresses of `alen` bytes (none for ICMP, protocol 1), stored at seg[field]. */
static inline void l4_checksum(uint8_t *seg, uint32_t sl, uint32_t field, const uint8_t *src, const uint8_t *dst, size_t alen,
                               uint8_t proto)
{
    put16(seg + field, 0);
    const uint16_t ph = proto == 1 ? 0 : (uint16_t)oracle_compute_pseudo_header_checksum(src, alen, dst, alen, sl, proto);
    put16(seg + field, 0xffffu ^ (uint32_t)oracle_compute_ones_comp(ph, seg, sl));
}

/* The addresses of a datagram on its way in. */
typedef struct rx_addrs {
    const uint8_t *remote4, *local4, *remote6, *local6;
} rx_addrs;

/* A valid datagram of kind k (0: IPv4 TCP, 1: IPv6 TCP, 2: IPv4 ICMP) and `len` random bytes in p. */
static inline void make_datagram(uint8_t *p, uint32_t len, int k, const rx_addrs *a)
{
    const uint32_t hdr = k == 1 ? 40 : 20;
    fill_random_bytes(p, len);
    memset(p, 0, hdr);
    if (k == 1) {
        ipv6_header(p, len - hdr, 6, a->remote6, a->local6);
        l4_checksum(p + hdr, len - hdr, 16, a->remote6, a->local6, 16, 6);
    } else {
        p[0] = 0x45; p[6] = 0x40; p[8] = 64; p[9] = k == 0 ? 6 : 1;
        ipv4_finish(p, 20, len, a->remote4, a->local4);
        l4_checksum(p + hdr, len - hdr, k == 2 ? 2 : 16, a->remote4, a->local4, 4, p[9]);
    }
}

/* The receive path over a datagram in the fragments (base, len)[0..n), the first one holding the IP
 * header: the header checksum, trim_head, the pseudo-header with the datagram's length,
 * compute_buffer_ones_comp over the trimmed fragments.  No fragments: header() asserts. */
enum { ABI_MAX_FRAGS = 8 };
static inline void rx_reference(const uint8_t *const *base, const size_t *len, size_t n, const uint8_t *local4,
                                const uint8_t *local6, uint8_t *status, uint16_t *l4)
{
    *l4 = 0;
    *status = RNS_RX_MALFORMED;
    if (n == 0 || n > ABI_MAX_FRAGS)
        return;
    const uint8_t *header = base[0], *tb[ABI_MAX_FRAGS];
    const int v6 = (header[0] >> 4) == 6;
    const uint32_t hdr = v6 ? 40 : (header[0] & 0xfu) * 4u;
    uint8_t st = (v6 || oracle_compute_checksum(header, hdr) == 0) ? RNS_RX_IP_OK : 0;
    const uint8_t proto = v6 ? header[6] : header[9];
    size_t tl[ABI_MAX_FRAGS], k = 0, total = 0;
    for (size_t f = 0; f < n; ++f) {
        const size_t cut = f == 0 ? hdr : 0;
        total += len[f];
        if (len[f] > cut) {
            tb[k] = base[f] + cut;
            tl[k++] = len[f] - cut;
        }
    }
    const uint16_t ph = proto == 1 ? 0
        : (uint16_t)oracle_compute_pseudo_header_checksum(header + (v6 ? 8 : 12), v6 ? 16 : 4, v6 ? local6 : local4,
                                                          v6 ? 16 : 4, total - hdr, proto);
    *l4 = (uint16_t)(0xffff ^ (k ? oracle_compute_buffer_ones_comp(ph, tb, tl, k) : ph));
    if (*l4 == 0)
        st |= RNS_RX_L4_OK;
    if ((st & RNS_RX_IP_OK) && (st & RNS_RX_L4_OK))
        st |= RNS_RX_ACCEPT;
    *status = st;
}

/* The same over a datagram of `total` bytes in the pool buffers idx[0..) of 1 << log2 bytes each, as
 * recv_packet leaves it (netif.rs:65-83). */
static inline void rx_reference_pool(const uint8_t *pool, uint32_t log2, const uint32_t *idx, uint32_t total,
                                     const uint8_t *local4, const uint8_t *local6, uint8_t *status, uint16_t *l4)
{
    const uint8_t *base[ABI_MAX_FRAGS];
    size_t len[ABI_MAX_FRAGS], n = 0;
    for (uint32_t pos = 0; pos < total && n < ABI_MAX_FRAGS; pos += 1u << log2, ++n) {
        base[n] = pool + ((uint64_t)idx[n] << log2);
        len[n] = total - pos < 1u << log2 ? total - pos : 1u << log2;
    }
    rx_reference(base, len, n, local4, local6, status, l4);
}

/* The head of segment j of a TCP send: the template t of hl bytes but for the lengths, id + j,
 * seq + j * mss; both checksums zero (tcp.rs:938-976, ip.rs:140-177). */
static inline void make_segment_head(uint8_t *h, const uint8_t *t, uint32_t hl, uint32_t j, uint32_t mss, uint32_t seglen)
{
    memcpy(h, t, hl);
    uint32_t iphdr = 40;
    if ((t[0] >> 4) == 4) {
        iphdr = 20;
        put16(h + 2, hl + seglen);
        put16(h + 4, get16(t + 4) + j);
        put16(h + 10, 0);
    } else {
        put16(h + 4, hl - 40 + seglen);
    }
    put32(h + iphdr + 4, get32(t + iphdr + 4) + j * mss);
    put16(h + iphdr + 16, 0);
}

#endif
