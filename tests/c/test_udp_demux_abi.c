/*
 * A plain C caller of the UDP receive demux (rns_rx_udp_demux_pool_dev, rns_rx_udp_demux_work,
 * rns_rx_udp_port_table_build), bound the way the reference's Rust would bind it (extern "C" + raw
 * pointers): no torch, no Python, the HIP runtime only for device memory.  1200 datagrams — UDP over IPv4
 * (with and without options) and IPv6 to 40 sockets and to unbound ports, TCP, and UDP behind a bad IPv4
 * header checksum — lie in shuffled 512-byte pool buffers as recv_packet leaves them.  The program queues
 * them itself the way udp_input does (udp.rs:126-148: a push_back per datagram onto its port's queue),
 * walks the sockets in order and compares every record and every payload byte, the flags, the positions,
 * d_q_first and d_count; then once more with too few records and too little room for the payloads.
 *
 * Prints "all checks passed" and exits 0 on success; exits 2 when no device memory can be had.
 */
#define ABI_TEST_SEED 0x0DB0F00Dull
#include "abi_test.h"

enum { N = 1200, LOG2 = 9, BUF = 1 << LOG2, MAXPAY = 1300, MAXT = 60 + 8 + MAXPAY, MAXFR = (MAXT + BUF - 1) / BUF,
       NRX = N * MAXFR, NBLK = (N + 63) / 64, SOCKS = 40, KINDS = 8, DATA = NRX * BUF };

static const uint8_t L4[4] = {10, 0, 0, 2}, R4[4] = {10, 0, 0, 1};
static const uint8_t L6[16] = {0xfe, 0x80, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2};
static const uint8_t R6[16] = {0xfe, 0x80, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};

/* A datagram of protocol `proto` with `pay` random bytes behind 8 bytes of ports, length and checksum:
 * IPv4 with IHL ihl (v6 == 0) or IPv6.  Its length. */
static uint32_t make_udp(uint8_t *d, int v6, uint32_t ihl, uint8_t proto, uint32_t sport, uint32_t dport, uint32_t pay)
{
    const uint32_t h = v6 ? 40 : 4 * ihl, T = h + 8 + pay;
    memset(d, 0, h + 8);
    fill_random_bytes(d + h + 8, pay);
    put16(d + h, sport);
    put16(d + h + 2, dport);
    put16(d + h + 4, (uint32_t)next_u64());  /* the length field and the checksum are not read */
    put16(d + h + 6, (uint32_t)next_u64());
    if (v6) {
        ipv6_header(d, 8 + pay, proto, R6, L6);
    } else {
        d[0] = (uint8_t)(0x40 | ihl); d[8] = 64; d[9] = proto;
        for (uint32_t b = 20; b < h; ++b)
            d[b] = 1;  /* options */
        ipv4_finish(d, h, T, R4, L4);
    }
    return T;
}

int main(void)
{
    static uint8_t rx[NRX * BUF], dg[N][MAXT], back[DATA], status[N], udp[N], want_udp[N];
    static uint16_t len16[N], ports[SOCKS], tbl[65536];
    static uint32_t idx[NRX], blk_first[NBLK], order[NRX], q_first[SOCKS + 1], pos[N], count[2], hdr[N], sock_of[N];
    static rns_udp_rec rec[N];
    for (uint32_t s = 0; s < SOCKS; ++s)
        ports[s] = (uint16_t)(7000 + 13 * s);
    shuffled_order(order, NRX);
    fill_random_bytes(rx, sizeof rx);
    uint32_t nf = 0, entries = 0;
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t edge[] = {0, 1, 15, 16, 17, BUF - 28, BUF - 27, BUF - 29, MAXPAY};
        const uint32_t k = i % KINDS, tcp = k == 7 && (i & 8);
        const uint32_t pay = i < 9 ? edge[i] : (tcp ? 12 : 0) + (uint32_t)(next_u64() % (i % 3 ? 90 : MAXPAY - 11));
        const uint32_t s = (uint32_t)(next_u64() % SOCKS), sport = 1024 + (uint32_t)(next_u64() % 60000);
        /* kinds: 0 2 4 IPv4, 1 5 IPv6, 3 IPv4 with options, 6 an unbound port, 7 TCP (its checksum verifies) or UDP
         * behind a bad header checksum */
        const uint32_t T = make_udp(dg[i], k == 1 || k == 5, k == 3 ? 6 + i % 10 : 5, tcp ? 6 : 17, sport,
                                    k == 6 ? 7001 : ports[s], pay);
        if (tcp)
            l4_checksum(dg[i] + 20, T - 20, 16, R4, L4, 4, 6);
        else if (k == 7)
            dg[i][10] ^= 0x20;
        sock_of[i] = k < 6 ? s : SOCKS;
        want_udp[i] = k < 6 ? RNS_UDP_DGRAM | RNS_UDP_SOCK : k == 6 ? RNS_UDP_DGRAM : 0;
        entries += k < 6;
        hdr[i] = (dg[i][0] >> 4) == 6 ? 40 : 4u * (dg[i][0] & 15);
        len16[i] = (uint16_t)T;
        if ((i & 63) == 0)
            blk_first[i >> 6] = nf;
        for (uint32_t at = 0; at < T; at += BUF, ++nf) {
            idx[nf] = order[nf];
            memcpy(rx + ((size_t)idx[nf] << LOG2), dg[i] + at, T - at < BUF ? T - at : BUF);
        }
    }

    /* the host helpers and every argument check need no device */
    uint64_t need = 0, need0 = 0;
    CHECK(rns_rx_udp_demux_work(N, SOCKS, NULL) == RNS_E_INVALID, "NULL bytes");
    CHECK(rns_rx_udp_demux_work(N, RNS_UDP_MAX_SOCKS + 1, &need) == RNS_E_INVALID, "too many sockets for the workspace");
    CHECK(rns_rx_udp_demux_work(0, 0, &need0) == RNS_OK && need0 > 0, "work(0, 0)");
    CHECK(rns_rx_udp_demux_work(N, SOCKS, &need) == RNS_OK && need >= need0, "work(N, SOCKS)");
    CHECK(rns_rx_udp_demux_work(1u << 20, 1024, &need0) == RNS_OK && need0 <= (64ull << 20), "work(2^20, 1024) = %llu",
          (unsigned long long)need0);
    CHECK(rns_rx_udp_port_table_build(ports, SOCKS, NULL) == RNS_E_INVALID, "NULL table");
    CHECK(rns_rx_udp_port_table_build(NULL, SOCKS, tbl) == RNS_E_INVALID, "NULL ports");
    CHECK(rns_rx_udp_port_table_build(ports, RNS_UDP_MAX_SOCKS + 1, tbl) == RNS_E_INVALID, "too many ports");
    ports[SOCKS - 1] = ports[3];
    CHECK(rns_rx_udp_port_table_build(ports, SOCKS, tbl) == RNS_E_INVALID, "a duplicate port");
    ports[SOCKS - 1] = (uint16_t)(7000 + 13 * (SOCKS - 1));
    CHECK(rns_rx_udp_port_table_build(ports, SOCKS, tbl) == RNS_OK, "the port table");
    for (uint32_t p = 0, s = 0; p < 65536; ++p) {
        const int bound = s < SOCKS && p == ports[s];
        CHECK(tbl[p] == (bound ? s : RNS_UDP_NO_SOCK), "tbl[%u] = %u", p, tbl[p]);
        s += (uint32_t)bound;
    }
    uint8_t *fake = (uint8_t *)4096;
#define CALL(pool, log2, nfr, n, tb, ns, data, db, rc, cap, qf, cnt, st, ud, wk, wkb)                                          \
    rns_rx_udp_demux_pool_dev(pool, sizeof rx, log2, (uint32_t *)fake, nfr, (uint32_t *)fake, (uint16_t *)fake, n, L4, L6, tb, ns, \
                              data, db, rc, cap, qf, cnt, st, NULL, ud, NULL, wk, wkb, NULL)
    rns_udp_rec *const frec = (rns_udp_rec *)fake;
    uint32_t *const f32 = (uint32_t *)fake;
    uint16_t *const f16 = (uint16_t *)fake;
    CHECK(CALL(NULL, LOG2, nf, N, f16, SOCKS, fake, DATA, frec, N, f32, f32, fake, fake, fake, need) == RNS_E_INVALID, "NULL pool");
    CHECK(CALL(fake + 8, LOG2, nf, N, f16, SOCKS, fake, DATA, frec, N, f32, f32, fake, fake, fake, need) == RNS_E_INVALID, "a misaligned pool");
    CHECK(CALL(fake, 6, nf, N, f16, SOCKS, fake, DATA, frec, N, f32, f32, fake, fake, fake, need) == RNS_E_INVALID, "buf_log2 6");
    CHECK(CALL(fake, 16, nf, N, f16, SOCKS, fake, DATA, frec, N, f32, f32, fake, fake, fake, need) == RNS_E_INVALID, "buf_log2 16");
    CHECK(CALL(fake, LOG2, 1u << 27, N, f16, SOCKS, fake, DATA, frec, N, f32, f32, fake, fake, fake, need) == RNS_E_INVALID, "2^36 buffer bytes");
    CHECK(CALL(fake, LOG2, nf, RNS_CHAIN_MAX_PACKETS + 1, f16, SOCKS, fake, DATA, frec, N, f32, f32, fake, fake, fake, ~0ull) == RNS_E_INVALID, "too many datagrams");
    CHECK(CALL(fake, LOG2, nf, N, NULL, SOCKS, fake, DATA, frec, N, f32, f32, fake, fake, fake, need) == RNS_E_INVALID, "NULL table with sockets");
    CHECK(CALL(fake, LOG2, nf, N, f16, RNS_UDP_MAX_SOCKS + 1, fake, DATA, frec, N, f32, f32, fake, fake, fake, ~0ull) == RNS_E_INVALID, "too many sockets");
    CHECK(CALL(fake, LOG2, nf, N, f16, SOCKS, NULL, DATA, frec, N, f32, f32, fake, fake, fake, need) == RNS_E_INVALID, "NULL data");
    CHECK(CALL(fake, LOG2, nf, N, f16, SOCKS, fake + 8, DATA, frec, N, f32, f32, fake, fake, fake, need) == RNS_E_INVALID, "misaligned data");
    CHECK(CALL(fake, LOG2, nf, N, f16, SOCKS, fake, DATA, NULL, N, f32, f32, fake, fake, fake, need) == RNS_E_INVALID, "NULL records");
    CHECK(CALL(fake, LOG2, nf, N, f16, SOCKS, fake, DATA, (rns_udp_rec *)(fake + 8), N, f32, f32, fake, fake, fake, need) == RNS_E_INVALID, "misaligned records");
    CHECK(CALL(fake, LOG2, nf, N, f16, SOCKS, fake, DATA, frec, N, NULL, f32, fake, fake, fake, need) == RNS_E_INVALID, "NULL q_first");
    CHECK(CALL(fake, LOG2, nf, N, f16, SOCKS, fake, DATA, frec, N, f32, NULL, fake, fake, fake, need) == RNS_E_INVALID, "NULL counts");
    CHECK(CALL(fake, LOG2, nf, N, f16, SOCKS, fake, DATA, frec, N, f32, f32, NULL, fake, fake, need) == RNS_E_INVALID, "NULL status");
    CHECK(CALL(fake, LOG2, nf, N, f16, SOCKS, fake, DATA, frec, N, f32, f32, fake, NULL, fake, need) == RNS_E_INVALID, "NULL d_udp");
    CHECK(CALL(fake, LOG2, nf, N, f16, SOCKS, fake, DATA, frec, N, f32, f32, fake, fake, NULL, need) == RNS_E_INVALID, "NULL workspace");
    CHECK(CALL(fake, LOG2, nf, N, f16, SOCKS, fake, DATA, frec, N, f32, f32, fake, fake, fake + 8, need) == RNS_E_INVALID, "a misaligned workspace");
    CHECK(CALL(fake, LOG2, nf, N, f16, SOCKS, fake, DATA, frec, N, f32, f32, fake, fake, fake, need - 1) == RNS_E_INVALID, "a short workspace");
    CHECK(CALL(fake, LOG2, nf, 0, f16, SOCKS, fake, DATA, frec, N, f32, NULL, fake, fake, fake, need) == RNS_E_INVALID, "no datagrams, NULL counts");

    /* udp_input, datagram by datagram: the queues as lists of datagram indices, socket-major */
    static uint32_t qlist[N], qn[SOCKS + 1];
    for (uint32_t i = 0; i < N; ++i)
        qn[sock_of[i]]++;
    uint32_t first[SOCKS + 1], fill[SOCKS + 1];
    for (uint32_t s = 0, at = 0; s <= SOCKS; ++s) {
        first[s] = fill[s] = at;
        at += s < SOCKS ? qn[s] : 0;
    }
    for (uint32_t i = 0; i < N; ++i)
        if (sock_of[i] < SOCKS)
            qlist[fill[sock_of[i]]++] = i;  /* push_back */

    uint8_t *d_rx = NULL, *d_status = NULL, *d_udp = NULL, *d_data = NULL;
    uint16_t *d_len = NULL, *d_tbl = NULL;
    uint32_t *d_idx = NULL, *d_blk = NULL, *d_qf = NULL, *d_count = NULL, *d_pos = NULL;
    rns_udp_rec *d_rec = NULL;
    void *d_work = NULL;
    hipStream_t st;
    UP(d_rx, rx, sizeof rx);
    UP(d_len, len16, sizeof len16);
    UP(d_idx, idx, sizeof idx);
    UP(d_blk, blk_first, sizeof blk_first);
    UP(d_tbl, tbl, sizeof tbl);
    OUT(d_status, N, 0);
    OUT(d_work, need, 0);
    HIP_OK(abi_stream(&st));
    for (int round = 0; round < 3; ++round) {
        /* round 1: records for the first 100 entries only; round 2: room for the payloads of the first 300 */
        uint32_t cap = N, units300 = 0;
        for (uint32_t k = 0; k < 300; ++k)
            units300 += (len16[qlist[k]] - hdr[qlist[k]] - 8u + 15u) / 16u;
        const uint64_t data_bytes = round == 2 ? 16ull * units300 : DATA;
        if (round == 1)
            cap = 100;
        OUT(d_data, DATA, 0xA5);
        OUT(d_rec, sizeof rec, 0xA5);
        OUT(d_udp, N, 0x55);
        OUT(d_pos, sizeof pos, 0x55);
        OUT(d_qf, sizeof q_first, 0x55);
        OUT(d_count, sizeof count, 0x55);
        CHECK(rns_rx_udp_demux_pool_dev(d_rx, sizeof rx, LOG2, d_idx, nf, d_blk, d_len, N, L4, L6, d_tbl, SOCKS, d_data, data_bytes,
                                        d_rec, cap, d_qf, d_count, d_status, NULL, d_udp, d_pos, d_work, need, st) == RNS_OK,
              "rns_rx_udp_demux_pool_dev");
        HIP_OK(hipStreamSynchronize(st));
        DOWN(count, d_count, sizeof count);
        DOWN(q_first, d_qf, sizeof q_first);
        DOWN(status, d_status, N);
        DOWN(udp, d_udp, N);
        DOWN(pos, d_pos, sizeof pos);
        DOWN(rec, d_rec, sizeof rec);
        DOWN(back, d_data, DATA);
        CHECK(count[0] == entries, "round %d: %u entries, %u expected", round, count[0], entries);
        for (uint32_t s = 0; s <= SOCKS; ++s)
            CHECK(q_first[s] == first[s], "round %d q_first[%u] = %u, not %u", round, s, q_first[s], first[s]);
        uint32_t off = 0;
        for (uint32_t k = 0; k < entries; ++k) {
            const uint32_t i = qlist[k], pay = len16[i] - hdr[i] - 8u, units = (pay + 15u) / 16u;
            const int queued = k < cap && 16ull * (off + units) <= data_bytes;
            const uint8_t flags = (uint8_t)(want_udp[i] | (queued ? RNS_UDP_QUEUED : RNS_UDP_NOROOM));
            CHECK(udp[i] == flags, "round %d udp[%u] = %02x, not %02x", round, i, udp[i], flags);
            CHECK(pos[i] == (queued ? k : 0xffffffffu), "round %d pos[%u] = %u (entry %u)", round, i, pos[i], k);
            const uint8_t *r = (const uint8_t *)&rec[k];
            if (queued) {
                const int v6 = hdr[i] == 40;
                uint8_t ip[16] = {0};
                memcpy(ip, v6 ? R6 : R4, v6 ? 16 : 4);
                CHECK(memcmp(rec[k].ip, ip, 16) == 0 && rec[k].family == (v6 ? 6 : 4), "round %d record %u: the source address", round, k);
                CHECK(rec[k].src == i && rec[k].off16 == off && rec[k].len == pay && rec[k].sport == get16(dg[i] + hdr[i]) &&
                          rec[k].flags == flags && rec[k].pad[0] == 0 && rec[k].pad[1] == 0,
                      "round %d record %u: src %u off16 %u len %u sport %u flags %02x", round, k, rec[k].src, rec[k].off16, rec[k].len,
                      rec[k].sport, rec[k].flags);
                CHECK(memcmp(back + 16ull * off, dg[i] + hdr[i] + 8, pay) == 0, "round %d entry %u (datagram %u): the payload differs", round, k, i);
            } else {
                for (uint32_t b = 0; b < 32; ++b)
                    CHECK(r[b] == 0xA5, "round %d: the record of cut entry %u written", round, k);
                for (uint64_t b = 16ull * off; b < 16ull * (off + units) && b < DATA; b += 7)
                    CHECK(back[b] == 0xA5, "round %d: the payload of cut entry %u written", round, k);
            }
            off += units;
        }
        CHECK(count[1] == off, "round %d: %u units, %u expected", round, count[1], off);
        for (uint64_t b = 16ull * off; b < DATA; b += 61)  /* past the queues: untouched */
            CHECK(back[b] == 0xA5, "round %d: data written past the last entry", round);
        for (uint32_t i = 0; i < N; ++i) {
            CHECK(((status[i] & RNS_RX_ACCEPT) != 0) == (i % KINDS != 7 || (i & 8)), "status[%u] = %02x", i, status[i]);
            if (sock_of[i] == SOCKS)
                CHECK(udp[i] == want_udp[i] && pos[i] == 0xffffffffu, "round %d udp[%u] = %02x pos %u", round, i, udp[i], pos[i]);
        }
    }
    return abi_finish("%d datagrams, %u queue entries over %d sockets", N, entries, SOCKS);
}
