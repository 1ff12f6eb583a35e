/*
 * A plain C caller of the TCP flow update (rns_rx_tcp_flow_update_dev, rns_rx_tcp_flow_update_work)
 * and the ACK build (rns_tx_ack_build_dev), bound the way the reference's Rust would bind them
 * (extern "C" + raw pointers): no torch, no Python, the HIP runtime only for device memory.
 * 300 meta records — the segments of four flows (IPv4, IPv6, IPv4, IPv6) interleaved at random,
 * mostly in order, some swapped with their neighbour, one flow stopped by a FIN half way, some
 * records of no flow between them — go through the update; the state, the results and every
 * d_seg record are checked against tcp.rs:642-740 restated here (a straight loop per flow), and
 * every ACK head against ip_output / tcp_output restated over the oracle's primitives
 * (oracle/csum_oracle.c, linked as test infrastructure only).
 *
 * Prints "all checks passed" and exits 0 on success; exits 2 when no device memory can be had.
 */
#define ABI_TEST_SEED 0xF10A5EEDull
#include "abi_test.h"

enum { N = 300, NFLOW = 4, CAP = 4, STRIDE = 64, ACKCAP = 64, FILL = 0xEE };

static int seq_le(uint32_t a, uint32_t b) { return !seq_gt(a, b); }

static rns_rx_tcp_meta meta[N];
static rns_tcp_flow flow_in[NFLOW], ref_flow[NFLOW], flow_out[NFLOW];
static uint32_t pend_in[NFLOW * CAP * 2], ref_pend[NFLOW * CAP * 2], pend_out[NFLOW * CAP * 2];
static rns_rx_tcp_seg ref_seg[N], seg[N];
static rns_tcp_flow_res ref_res[NFLOW], res[NFLOW];
static uint8_t tmpl[NFLOW * STRIDE], head_len8[NFLOW], out[ACKCAP * 64], ack_len8[ACKCAP];
static uint32_t ack_src[ACKCAP], n_acks[2];
static const uint8_t local4[4] = {192, 168, 1, 1};
static const uint8_t local6[16] = {0xfe, 0x80, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};

/* tcp.rs:642-740 for flow f over its records in batch order, with the stops of rns_checksum.h */
static void update_ref(uint32_t f)
{
    rns_tcp_flow s = flow_in[f];
    rns_tcp_flow_res r = {0, 0, 0xffffffffu, 0, 0, 0, 0, RNS_STOP_NONE};
    uint32_t *pend = ref_pend + f * CAP * 2;
    memcpy(pend, pend_in + f * CAP * 2, sizeof(uint32_t) * CAP * 2);
    for (uint32_t i = 0; i < N; ++i)
        if ((meta[i].place & RNS_PLACE_FLOW) && meta[i].flow == f)
            r.n_segs++;
    for (uint32_t i = 0; i < N && r.why == RNS_STOP_NONE; ++i) {
        const rns_rx_tcp_meta *m = &meta[i];
        if (!(m->place & RNS_PLACE_FLOW) || m->flow != f)
            continue;
        if (m->flags & 0x07)
            r.why = RNS_STOP_FLAGS;
        else if (m->tcp_hdr != 20)
            r.why = RNS_STOP_OPTIONS;
        else if (m->place & RNS_PLACE_OUTSIDE)
            r.why = RNS_STOP_OUTSIDE;
        else if (m->pay_len && m->seq != s.rcv_nxt && s.n_pend == CAP)
            r.why = RNS_STOP_PEND;
        if (r.why != RNS_STOP_NONE) {
            r.stop = i;
            break;
        }
        ref_seg[i].act = RNS_SEG_CONSUMED;
        if (m->pay_len) {
            uint32_t end = m->seq + m->pay_len, got = 0;
            if (!seq_gt(s.rcv_max, end))
                s.rcv_max = end;
            if (m->seq == s.rcv_nxt) {
                got = m->pay_len;
                s.rcv_nxt += m->pay_len;
                for (uint32_t k = 0; k < s.n_pend;) {
                    int before = seq_gt(m->seq, pend[2 * k]);
                    if (before || pend[2 * k] == s.rcv_nxt) {
                        uint32_t ln = pend[2 * k + 1];
                        memmove(pend + 2 * k, pend + 2 * k + 2, sizeof(uint32_t) * 2 * (s.n_pend - k - 1));
                        s.n_pend--;
                        if (!before) {
                            s.rcv_nxt += ln;
                            got += ln;
                            k = 0;
                        }
                    } else {
                        k++;
                    }
                }
            } else {
                pend[2 * s.n_pend] = m->seq;
                pend[2 * s.n_pend + 1] = m->pay_len;
                s.n_pend++;
            }
            s.rq_len += got;
            r.readable += got;
            if (++s.delayed_acks >= 5) {
                s.delayed_acks = 0;
                s.ack_timer = 0;
                ref_seg[i].act |= RNS_SEG_ACK;
                ref_seg[i].ack_num = s.rcv_nxt;
                ref_seg[i].window = (uint16_t)(0xffffu - (s.rq_len & 0xffffu));
                r.n_acks++;
            } else if (!s.ack_timer) {
                s.ack_timer = 1;
                ref_seg[i].act |= RNS_SEG_TIMER;
            }
        }
        if (m->flags & 0x10) {
            if (seq_gt(m->ack, s.snd_una) && seq_le(m->ack, s.snd_nxt)) {
                r.acked += m->ack - s.snd_una;
                s.snd_una = m->ack;
            }
            if (seq_le(s.snd_una, m->ack) && seq_le(m->ack, s.snd_nxt) &&
                (seq_gt(m->seq, s.snd_wl1) || (s.snd_wl1 == m->seq && seq_le(s.snd_wl2, m->ack)))) {
                s.snd_wnd = m->window;
                s.snd_wl1 = m->seq;
                s.snd_wl2 = m->ack;
                r.events |= RNS_EV_WND;
            }
        }
        r.consumed++;
    }
    ref_flow[f] = s;
    ref_res[f] = r;
}

/* tcp_output (tcp.rs:938-976) and ip_output (ip.rs:140-177) for a pure ACK of flow f; returns the head length */
static uint32_t ack_ref(uint32_t f, uint32_t ack_num, uint32_t window, uint32_t id, uint8_t *h)
{
    const int v4 = head_len8[f] == 40;
    const uint32_t ip = v4 ? 20 : 40;
    memcpy(h, tmpl + f * STRIDE, ip + 20);
    uint8_t *t = h + ip;
    put32(t + 4, ref_flow[f].snd_nxt);
    put32(t + 8, ack_num);
    t[12] = 0x50, t[13] = 0x10;
    put16(t + 14, window);
    put16(t + 16, 0);
    int32_t ph = v4 ? oracle_compute_pseudo_header_checksum(h + 12, 4, h + 16, 4, 20, 6)
                    : oracle_compute_pseudo_header_checksum(h + 8, 16, h + 24, 16, 20, 6);
    put16(t + 16, (uint32_t)oracle_compute_ones_comp((uint16_t)ph, t, 20) ^ 0xffffu);
    if (v4) {
        put16(h + 2, 40);
        put16(h + 4, id);
        put16(h + 10, 0);
        put16(h + 10, (uint32_t)oracle_compute_checksum(h, 20));
    } else {
        put16(h + 4, 20);
    }
    return ip + 20;
}

int main(void)
{
    /* the flows and their templates: junk in every field the build writes */
    uint32_t next[NFLOW], sent[NFLOW] = {0};
    for (uint32_t f = 0; f < NFLOW; ++f) {
        const int v4 = (f & 1) == 0;
        uint8_t *t = tmpl + f * STRIDE;
        memset(t, 0x5A + f, STRIDE);
        head_len8[f] = v4 ? 40 : 60;
        if (v4) {
            t[0] = 0x45, t[1] = 0, t[6] = t[7] = 0, t[8] = 64, t[9] = 6;
            memcpy(t + 12, local4, 4);
            t[16] = 10, t[17] = 0, t[18] = 0, t[19] = (uint8_t)(f + 2);
        } else {
            t[0] = 0x60, t[1] = t[2] = t[3] = 0, t[6] = 6, t[7] = 64;
            memcpy(t + 8, local6, 16);
            memset(t + 24, 0x20 + f, 16);
        }
        uint8_t *tcp = t + (v4 ? 20 : 40);
        put16(tcp, 80), put16(tcp + 2, 4000 + f);
        tcp[12] = 0x5F;
        put16(tcp + 18, 0);
        memset(&flow_in[f], 0, sizeof flow_in[f]);
        next[f] = f == 1 ? 0xFFFFFF00u : 100000u * (f + 1);
        flow_in[f].rcv_nxt = flow_in[f].rcv_max = next[f];
        flow_in[f].snd_una = 5000, flow_in[f].snd_nxt = 20000 + f, flow_in[f].snd_wl1 = next[f] - 1;
        flow_in[f].rq_len = 11 * f, flow_in[f].delayed_acks = (uint16_t)f, flow_in[f].state = RNS_TCP_ESTABLISHED;
    }
    flow_in[3].snd_nxt = 7000; /* later ACK numbers are beyond it */
    memset(pend_in, 0, sizeof pend_in);
    int fin_sent = 0;
    for (uint32_t i = 0; i < N; ++i) {
        rns_rx_tcp_meta *m = &meta[i];
        memset(m, 0, sizeof *m);
        const uint32_t f = (uint32_t)(next_u64() % (NFLOW + 1));
        if (f == NFLOW) { /* not a flow's: undecoded, unmatched, or a flow index past the table */
            const uint32_t kind = i % 3;
            m->flow = kind == 2 ? 77 : RNS_RX_NO_FLOW;
            m->place = kind == 0 ? 0 : kind == 1 ? RNS_PLACE_TCP : RNS_PLACE_TCP | RNS_PLACE_FLOW;
            m->seq = 1, m->flags = 0x10, m->tcp_hdr = 20;
            continue;
        }
        const uint32_t ln = next_u64() % 5 == 0 ? 0 : 1 + (uint32_t)(next_u64() % 1400);
        m->flow = f, m->seq = next[f] + sent[f], m->ack = 5000 + 13 * i, m->sport = (uint16_t)(4000 + f), m->dport = 80;
        m->window = (uint16_t)(1000 + i), m->pay_len = (uint16_t)ln, m->flags = ln ? 0x18 : 0x10;
        m->ip_hdr = (f & 1) ? 40 : 20, m->tcp_hdr = 20;
        m->place = RNS_PLACE_TCP | RNS_PLACE_FLOW | (ln ? RNS_PLACE_DONE : 0);
        sent[f] += ln;
        if (f == 2 && i > N / 2 && !fin_sent) { /* one FIN stops flow 2 half way */
            m->flags |= 0x01;
            fin_sent = 1;
        }
    }
    for (uint32_t i = 10; i + 1 < N; i += 17) { /* out of order: a segment swapped with the flow's next one */
        uint32_t j = i + 1;
        while (j < N && !(meta[j].flow == meta[i].flow && (meta[j].place & RNS_PLACE_FLOW)))
            j++;
        if (j < N && (meta[i].place & RNS_PLACE_FLOW) && meta[i].flow < NFLOW) {
            rns_rx_tcp_meta t = meta[i];
            meta[i] = meta[j];
            meta[j] = t;
        }
    }
    memset(ref_seg, 0, sizeof ref_seg);
    for (uint32_t f = 0; f < NFLOW; ++f)
        update_ref(f);
    uint32_t total_acks = 0, stopped = 0, pended = 0;
    for (uint32_t f = 0; f < NFLOW; ++f) {
        total_acks += ref_res[f].n_acks;
        stopped += ref_res[f].why != RNS_STOP_NONE;
    }
    for (uint32_t i = 0; i < N; ++i)
        pended += (ref_seg[i].act & RNS_SEG_CONSUMED) && meta[i].pay_len && !(ref_seg[i].act & (RNS_SEG_ACK | RNS_SEG_TIMER));
    CHECK(total_acks >= 20 && total_acks <= ACKCAP && stopped == 1 && ref_res[2].why == RNS_STOP_FLAGS && pended > 50,
          "the batch: %u ACKs, %u stopped", total_acks, stopped);

    /* argument checks, before the device is touched */
    uint64_t need = 0, need0 = 0;
    void *fake = (void *)(uintptr_t)4096;
    CHECK(rns_rx_tcp_flow_update_work(N, NFLOW, &need) == RNS_OK && need >= 4 * (N + 2 * NFLOW), "work: %llu",
          (unsigned long long)need);
    CHECK(rns_rx_tcp_flow_update_work(0, 0, &need0) == RNS_OK && need0 <= need, "work is monotone");
    CHECK(rns_rx_tcp_flow_update_work(N, NFLOW, NULL) == RNS_E_INVALID, "NULL bytes");
    CHECK(rns_rx_tcp_flow_update_dev(NULL, 0, 0, NULL, NULL, 0, NULL, NULL, NULL, NULL, NULL, 0, NULL) == RNS_OK, "empty");
    CHECK(rns_rx_tcp_flow_update_dev(fake, N, NFLOW, fake, fake, CAP, fake, fake, fake, fake, fake, need - 1, NULL) ==
              RNS_E_INVALID, "a short workspace");
    CHECK(rns_rx_tcp_flow_update_dev(fake, N, NFLOW, fake, NULL, CAP, fake, fake, fake, fake, fake, need, NULL) ==
              RNS_E_INVALID, "NULL d_pend_in");
    CHECK(rns_tx_ack_build_dev(fake, fake, N, fake, NFLOW, fake, STRIDE, fake, 0, fake, need, fake, ACKCAP, fake, fake, NULL,
                               NULL) == RNS_E_INVALID, "NULL d_n_acks");

    rns_rx_tcp_meta *d_meta = NULL;
    rns_tcp_flow *d_fin = NULL, *d_fout = NULL;
    uint32_t *d_pin = NULL, *d_pout = NULL, *d_src = NULL, *d_n = NULL;
    rns_rx_tcp_seg *d_seg = NULL;
    rns_tcp_flow_res *d_res = NULL;
    uint8_t *d_work = NULL, *d_tmpl = NULL, *d_hl = NULL, *d_out = NULL, *d_len = NULL;
    UP(d_meta, meta, sizeof meta);
    UP(d_fin, flow_in, sizeof flow_in);
    UP(d_pin, pend_in, sizeof pend_in);
    UP(d_tmpl, tmpl, sizeof tmpl);
    UP(d_hl, head_len8, sizeof head_len8);
    OUT(d_work, need, FILL);
    OUT(d_fout, sizeof flow_out, FILL);
    OUT(d_pout, sizeof pend_out, FILL);
    OUT(d_seg, sizeof seg, FILL);
    OUT(d_res, sizeof res, FILL);
    OUT(d_out, sizeof out, FILL);
    OUT(d_src, sizeof ack_src, FILL);
    OUT(d_len, sizeof ack_len8, FILL);
    OUT(d_n, sizeof n_acks, FILL);

    CHECK(rns_rx_tcp_flow_update_dev(d_meta, N, NFLOW, d_fin, d_pin, CAP, d_fout, d_pout, d_seg, d_res, d_work, need, NULL) ==
              RNS_OK, "rns_rx_tcp_flow_update_dev");
    CHECK(rns_tx_ack_build_dev(d_meta, d_seg, N, d_fout, NFLOW, d_tmpl, STRIDE, d_hl, 0xFFF0, d_work, need, d_out, ACKCAP,
                               d_src, d_len, d_n, NULL) == RNS_OK, "rns_tx_ack_build_dev");
    HIP_OK(hipDeviceSynchronize());
    DOWN(flow_out, d_fout, sizeof flow_out);
    DOWN(pend_out, d_pout, sizeof pend_out);
    DOWN(seg, d_seg, sizeof seg);
    DOWN(res, d_res, sizeof res);
    DOWN(out, d_out, sizeof out);
    DOWN(ack_src, d_src, sizeof ack_src);
    DOWN(ack_len8, d_len, sizeof ack_len8);
    DOWN(n_acks, d_n, sizeof n_acks);

    for (uint32_t f = 0; f < NFLOW; ++f) {
        CHECK(memcmp(&flow_out[f], &ref_flow[f], sizeof flow_out[f]) == 0, "flow %u: rcv_nxt %u != %u, n_pend %u != %u", f,
              flow_out[f].rcv_nxt, ref_flow[f].rcv_nxt, flow_out[f].n_pend, ref_flow[f].n_pend);
        CHECK(memcmp(&res[f], &ref_res[f], sizeof res[f]) == 0, "result %u: consumed %u != %u, why %u != %u", f,
              res[f].consumed, ref_res[f].consumed, res[f].why, ref_res[f].why);
        CHECK(memcmp(pend_out + f * CAP * 2, ref_pend + f * CAP * 2, 8 * ref_flow[f].n_pend) == 0, "pending list %u", f);
    }
    for (uint32_t i = 0; i < N; ++i)
        CHECK(memcmp(&seg[i], &ref_seg[i], sizeof seg[i]) == 0, "seg %u: act %u != %u, ack %u != %u", i, seg[i].act,
              ref_seg[i].act, seg[i].ack_num, ref_seg[i].ack_num);

    uint32_t k = 0, k4 = 0;
    for (uint32_t i = 0; i < N; ++i) {
        if (!(ref_seg[i].act & RNS_SEG_ACK))
            continue;
        uint8_t h[64];
        const uint32_t f = meta[i].flow, hl = ack_ref(f, ref_seg[i].ack_num, ref_seg[i].window, (0xFFF0u + k4) & 0xffffu, h);
        CHECK(ack_src[k] == i && ack_len8[k] == hl, "ACK %u: datagram %u != %u, length %u != %u", k, ack_src[k], i,
              ack_len8[k], hl);
        CHECK(memcmp(out + 64 * k, h, hl) == 0, "ACK %u of flow %u: head bytes", k, f);
        for (uint32_t b = hl; b < 64; ++b)
            CHECK(out[64 * k + b] == FILL, "ACK %u: byte %u of the slot's tail written", k, b);
        k4 += hl == 40;
        k++;
    }
    CHECK(n_acks[0] == k && n_acks[1] == k4 && k == total_acks && k4 > 5, "counts %u %u != %u %u", n_acks[0], n_acks[1], k, k4);
    for (uint32_t b = 64 * k; b < sizeof out; ++b)
        CHECK(out[b] == FILL, "byte %u past the last ACK written", b);

    return abi_finish("%d records of %d flows, %u ACKs", N, NFLOW, k);
}
