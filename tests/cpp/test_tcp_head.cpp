// The shared TCP head builder (csrc/rns_k_tcp_head.hpp) on the host: every patched byte against the
// field values written out by hand, the IPv4 header checksum and the TCP checksum against the oracle's
// one's-complement sum, and the template rule's rejections.
#include <cstdio>
#include <cstring>
#include <vector>

#include "rns_k_tcp_head.hpp"

extern "C" int32_t oracle_compute_ones_comp(uint16_t in_checksum, const uint8_t *slice, size_t len);

using namespace rns;

static int g_fail = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            if (++g_fail <= 20) {                             \
                std::fprintf(stderr, "line %d: ", __LINE__);  \
                std::fprintf(stderr, __VA_ARGS__);            \
                std::fprintf(stderr, "\n");                   \
            }                                                 \
        }                                                     \
    } while (0)

static void be16(uint8_t *b, uint32_t v) { b[0] = static_cast<uint8_t>(v >> 8), b[1] = static_cast<uint8_t>(v); }
static void be32(uint8_t *b, uint32_t v) { be16(b, v >> 16), be16(b + 2, v & 0xffffu); }

// A template head: every field the builder writes holds 0xa5 bytes, the rest what a flow's head holds.
static std::vector<uint8_t> make_tmpl(bool v4, uint32_t stride)
{
    std::vector<uint8_t> t(stride, 0xa5);
    const uint32_t ip = v4 ? 20 : 40;
    if (v4) {
        t[0] = 0x45, t[1] = 0, t[6] = 0x40, t[7] = 0, t[8] = 64, t[9] = 6;
        for (uint32_t k = 0; k < 8; ++k)
            t[12 + k] = static_cast<uint8_t>(0xc0 + 7 * k);
    } else {
        t[0] = 0x60, t[1] = 0x01, t[2] = 0x23, t[3] = 0x45, t[6] = 6, t[7] = 64;
        for (uint32_t k = 0; k < 32; ++k)
            t[8 + k] = static_cast<uint8_t>(0x20 + 5 * k);
    }
    be16(&t[ip], 0x1234), be16(&t[ip + 2], 0xfedc);  // the ports
    t[ip + 12] = 0x50;
    t[ip + 18] = 0, t[ip + 19] = 0;  // the urgent pointer
    return t;
}

struct Fields {
    uint32_t id, seq, ack, window, flags;
};

// The head at o (any alignment) from the template through the shared patch, sums and store; fin as
// tcp_head_patch takes it.  Returns the sums (of use with fin, the checksum fields being zero then).
static TcpHeadSum build(const uint8_t *t, uint8_t *o, uint32_t hl, const Fields &f, bool fin, uint32_t pay)
{
    const bool v4 = hl == 40, al4 = (reinterpret_cast<uintptr_t>(o) & 3) == 0;
    const uint32_t ipd = v4 ? 5 : 10;
    TcpHeadSum hs;
    for (uint32_t k = 0; k < hl / 4; ++k) {
        uint32_t d;
        std::memcpy(&d, t + 4 * k, 4);
        d = tcp_head_patch(k, d, v4, ipd, f.id, f.seq, f.ack, f.window, f.flags, fin, pay);
        hs.add(k, d, v4, ipd);
        store_dword(o + 4 * k, d, al4);
    }
    return hs;
}

// The fields by hand into e, a copy of the template.
static void expect(std::vector<uint8_t> &e, uint32_t hl, const Fields &f, bool fin, uint32_t pay)
{
    const bool v4 = hl == 40;
    const uint32_t ip = v4 ? 20 : 40;
    if (v4)
        be16(&e[4], f.id);
    if (fin) {
        if (v4) {
            be16(&e[2], 40 + pay);
            e[10] = e[11] = 0;
        } else {
            be16(&e[4], 20 + pay);
        }
        e[ip + 16] = e[ip + 17] = 0;
    }
    be32(&e[ip + 4], f.seq);
    be32(&e[ip + 8], f.ack);
    e[ip + 12] = 0x50;
    e[ip + 13] = static_cast<uint8_t>(f.flags);
    be16(&e[ip + 14], f.window);
}

// One finished head: bytes, then both checksums filled as the kernels fill them and verified.
static void check_final(bool v4, const Fields &f, uint32_t pay, uint32_t misalign, bool via_plan)
{
    const uint32_t hl = v4 ? 40 : 60, ip = v4 ? 20 : 40;
    const std::vector<uint8_t> t = make_tmpl(v4, 64);
    std::vector<uint8_t> buf(72, 0xee), e = t;
    uint8_t *o = buf.data() + misalign;
    TcpHeadSum hs;
    if (via_plan) {  // the planner's row first, lengths and checksums left to the second step
        std::vector<uint8_t> row(64, 0xee), er = t;
        (void)build(t.data(), row.data(), hl, f, false, 0);
        expect(er, hl, f, false, 0);
        CHECK(std::memcmp(row.data(), er.data(), hl) == 0, "plan row v4=%d id=%x seq=%x ack=%x", v4, f.id, f.seq, f.ack);
        CHECK(row[hl] == 0xee, "plan row written past the head");
        hs = build(row.data(), o, hl, f, true, pay);
    } else {
        hs = build(t.data(), o, hl, f, true, pay);
    }
    expect(e, hl, f, true, pay);
    CHECK(std::memcmp(o, e.data(), hl) == 0, "head v4=%d id=%x seq=%x ack=%x win=%x pay=%u", v4, f.id, f.seq, f.ack, f.window, pay);
    CHECK(buf[misalign + hl] == 0xee && (misalign == 0 || buf[misalign - 1] == 0xee), "stored outside the head");

    // the payload's big-endian sum onto the head's, as the segmentation folds it
    std::vector<uint8_t> p(pay);
    for (uint32_t k = 0; k < pay; ++k)
        p[k] = static_cast<uint8_t>(k * 131u + 17u + f.id);
    const uint32_t psum = pay ? static_cast<uint32_t>(oracle_compute_ones_comp(0, p.data(), pay)) : 0u;
    const uint32_t l4 = fold16(hs.l4_head(20 + pay) + psum) ^ 0xffffu;
    if (v4)
        be16(o + 10, hs.ip_csum());
    be16(o + ip + 16, l4);

    if (v4)
        CHECK(oracle_compute_ones_comp(0, o, 20) == 0xffff, "IPv4 header checksum id=%x pay=%u", f.id, pay);
    std::vector<uint8_t> ph;  // pseudo-header, TCP header, payload
    if (v4) {
        ph.assign(o + 12, o + 20);
        ph.resize(12, 0);
        ph[9] = 6;
        be16(&ph[10], 20 + pay);
    } else {
        ph.assign(o + 8, o + 40);
        ph.resize(ph.size() + 8, 0);
        be32(&ph[32], 20 + pay);
        ph[39] = 6;
    }
    ph.insert(ph.end(), o + ip, o + hl);
    ph.insert(ph.end(), p.begin(), p.end());
    CHECK(oracle_compute_ones_comp(0, ph.data(), ph.size()) == 0xffff, "TCP checksum v4=%d seq=%x ack=%x win=%x pay=%u", v4,
          f.seq, f.ack, f.window, pay);
}

static void check_rule()
{
    for (int v = 0; v < 2; ++v) {
        const bool v4 = v == 0;
        const uint32_t hl = v4 ? 40 : 60, ip = v4 ? 20 : 40;
        const std::vector<uint8_t> good = make_tmpl(v4, 64);
        CHECK(tcp_tmpl_ok(good.data(), hl, 64), "a good template v4=%d", v4);
        CHECK(tcp_tmpl_ok(good.data(), hl, hl), "stride == head length v4=%d", v4);
        CHECK(!tcp_tmpl_ok(good.data(), hl, hl - 1), "stride below the head length v4=%d", v4);
        CHECK(!tcp_tmpl_ok(good.data(), 41, 64), "length 41");
        std::vector<uint8_t> t = good;
        t[0] = static_cast<uint8_t>(0x50 | (t[0] & 0xf));
        CHECK(!tcp_tmpl_ok(t.data(), hl, 64), "version 5 v4=%d", v4);
        t = good;
        t[v4 ? 9 : 6] = 17;
        CHECK(!tcp_tmpl_ok(t.data(), hl, 64), "protocol 17 v4=%d", v4);
        t = good;
        t[ip + 12] = 0x60;
        CHECK(!tcp_tmpl_ok(t.data(), hl, 64), "data offset 6 v4=%d", v4);
    }
    const std::vector<uint8_t> six = make_tmpl(false, 64);
    CHECK(!tcp_tmpl_ok(six.data(), 40, 64), "an IPv6 template at head length 40");
}

int main()
{
    const uint32_t ids[] = {0, 1, 0xffff}, seqs[] = {0, 0x7fffffffu, 0xffffffffu}, wins[] = {0, 0xffff};
    const uint32_t pays[] = {0, 1, 2, 1459, 1460};
    CHECK(bswap16_u32(0x1234) == 0x3412 && be2(0x44332211u) == 0x1122u + 0x3344u && fold16(0x1ffffu) == 1u &&
              fold16(0xffffu) == 0xffffu,
          "byte-order helpers");
    int n = 0;
    for (int v = 0; v < 2; ++v)
        for (uint32_t id : ids)
            for (uint32_t seq : seqs)
                for (uint32_t ack : seqs)
                    for (uint32_t win : wins) {
                        const uint32_t mis = static_cast<uint32_t>(n++ % 4);  // the store at every alignment
                        check_final(v == 0, Fields{id, seq, ack, win, 0x10}, 0, mis, false);  // the ACK form
                        for (uint32_t pay : pays)  // the planner's row, then a segment of it
                            check_final(v == 0, Fields{id, seq, ack, win, 0x18}, pay, mis, true);
                    }
    check_rule();
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed (%d field sets)\n", n);
    return 0;
}
