/*
 * A plain C caller of the TCP connection update (rns_rx_tcp_conn_update_dev, rns_rx_tcp_conn_update_work), the
 * control-segment build (rns_tx_tcp_ctl_build_dev, rns_tx_tcp_ctl_build_work) and the close step
 * (rns_tx_tcp_close_dev), bound the way the reference's Rust would bind them: every argument
 * error of the five symbols before the device is touched, then two hand-traced lifecycles (tcp.rs:195-224,
 * 402-447, 622-835) as one stream of launches — passive open, request, the peer's FIN, our close, the last
 * ACK; and our close first, the ACK of our FIN, the peer's FIN — with every control segment's bytes rebuilt
 * over the oracle's checksum primitives.
 */
#define ABI_TEST_SEED 0x7C9C0221ull
#include "abi_test.h"

enum { NFLOW = 3, N1 = 5, CAP = 2, STRIDE = 64, FILL = 0xEE };

static const uint8_t local4[4] = {10, 0, 0, 1}, local6[16] = {0x20, 0x01, 0x0d, 0xb8, [15] = 1};
static uint8_t tmpl[NFLOW * STRIDE], head_len8[NFLOW];

/* The control segment of record c over its flow's template, as tcp_output and ip_output build it. */
static uint32_t ctl_ref(const rns_tcp_ctl *c, uint32_t id, uint8_t *h)
{
    const uint32_t f = c->flow;
    const int v4 = head_len8[f] == 40;
    const uint32_t ip = v4 ? 20 : 40;
    memcpy(h, tmpl + f * STRIDE, ip + 20);
    uint8_t *t = h + ip;
    put32(t + 4, c->seq);
    put32(t + 8, c->ack_num);
    t[12] = 0x50, t[13] = c->flags;
    put16(t + 14, c->window);
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

static rns_rx_tcp_meta seg_of(uint32_t flow, uint32_t seq, uint32_t ack, uint16_t pay, uint8_t flags)
{
    rns_rx_tcp_meta m;
    memset(&m, 0, sizeof m);
    m.flow = flow, m.seq = seq, m.ack = ack, m.sport = (uint16_t)(4000 + flow), m.dport = 80, m.window = 8192;
    m.pay_len = pay, m.flags = flags, m.ip_hdr = head_len8[flow] == 40 ? 20 : 40, m.tcp_hdr = 20;
    m.place = RNS_PLACE_TCP | RNS_PLACE_FLOW | (pay ? RNS_PLACE_DONE : 0);
    return m;
}

int main(void)
{
    for (uint32_t f = 0; f < NFLOW; ++f) { /* templates: junk in every field the build writes */
        const int v4 = f != 1;
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
    }
    /* flow 0: an accept record (SynReceived: snd_una holds the peer's number); flows 1, 2: Established */
    rns_tcp_flow fl[NFLOW];
    memset(fl, 0, sizeof fl);
    fl[0].rcv_nxt = fl[0].rcv_max = 101, fl[0].snd_una = 100, fl[0].snd_nxt = 9000, fl[0].snd_wnd = 8192, fl[0].snd_wl1 = 100;
    fl[0].state = RNS_TCP_SYN_RECEIVED;
    for (uint32_t f = 1; f < NFLOW; ++f) {
        fl[f].rcv_nxt = fl[f].rcv_max = 500, fl[f].snd_una = fl[f].snd_nxt = 7000, fl[f].snd_wnd = 1000, fl[f].snd_wl1 = 499;
        fl[f].snd_wl2 = 7000, fl[f].state = RNS_TCP_ESTABLISHED;
    }
    /* batch 1: flow 0's third ACK, request and FIN; flow 2 gets an RST in between */
    const rns_rx_tcp_meta b1[N1] = {seg_of(0, 101, 9001, 0, 0x10), seg_of(2, 500, 7000, 4, 0x18), seg_of(0, 101, 9001, 20, 0x18),
                                    seg_of(2, 77, 0, 0, 0x04), seg_of(0, 121, 9001, 0, 0x11)};
    const uint8_t act1[N1] = {RNS_CTL_CONSUMED | RNS_CTL_STATE, RNS_CTL_CONSUMED | RNS_CTL_ACK_TIMER,
                              RNS_CTL_CONSUMED | RNS_CTL_ACK_TIMER, RNS_CTL_CONSUMED | RNS_CTL_RESET | RNS_CTL_STATE,
                              RNS_CTL_CONSUMED | RNS_CTL_STATE};
    const uint8_t op[NFLOW] = {1, 1, 1};
    /* batch 2: the last ACK of flow 0; the ACK of flow 1's FIN, then the peer's FIN */
    enum { N2 = 3 };
    const rns_rx_tcp_meta b2[N2] = {seg_of(1, 500, 7001, 0, 0x10), seg_of(0, 122, 9002, 0, 0x10), seg_of(1, 500, 7001, 0, 0x11)};

    /* argument checks, before the device is touched */
    uint64_t need = 0, need0 = 0, bneed = 0, bneed0 = 0;
    void *fake = (void *)(uintptr_t)4096, *odd = (void *)(uintptr_t)4098;
    CHECK(rns_rx_tcp_conn_update_work(N1, NFLOW, &need) == RNS_OK && need >= 4 * (N1 + 2 * NFLOW), "work: %llu",
          (unsigned long long)need);
    CHECK(rns_rx_tcp_conn_update_work(0, 0, &need0) == RNS_OK && need0 <= need, "work is monotone");
    CHECK(rns_rx_tcp_conn_update_work(N1, NFLOW, NULL) == RNS_E_INVALID, "NULL bytes");
    CHECK(rns_rx_tcp_conn_update_work(N1, 0x80000000u, &need0) == RNS_E_INVALID, "too many flows");
    CHECK(rns_tx_tcp_ctl_build_work(N1, &bneed) == RNS_OK && bneed > 0 && bneed <= need, "build work: %llu",
          (unsigned long long)bneed);
    CHECK(rns_tx_tcp_ctl_build_work(0, &bneed0) == RNS_OK && bneed0 > 0 && bneed0 <= bneed, "build work is monotone");
    CHECK(rns_tx_tcp_ctl_build_work(N1, NULL) == RNS_E_INVALID, "NULL bytes");
    CHECK(rns_rx_tcp_conn_update_dev(NULL, 0, 0, NULL, NULL, 0, NULL, NULL, NULL, NULL, NULL, 0, NULL) == RNS_OK, "empty");
    CHECK(rns_rx_tcp_conn_update_dev(fake, N1, NFLOW, fake, fake, CAP, fake, fake, fake, fake, fake, need - 1, NULL) ==
              RNS_E_INVALID, "a short workspace");
    CHECK(rns_rx_tcp_conn_update_dev(fake, N1, NFLOW, fake, NULL, CAP, fake, fake, fake, fake, fake, need, NULL) ==
              RNS_E_INVALID, "NULL d_pend_in");
    CHECK(rns_rx_tcp_conn_update_dev(fake, N1, NFLOW, fake, fake, CAP, fake, fake, NULL, fake, fake, need, NULL) ==
              RNS_E_INVALID, "NULL d_ctl");
    CHECK(rns_rx_tcp_conn_update_dev(fake, N1, NFLOW, fake, fake, CAP, fake, fake, odd, fake, fake, need, NULL) ==
              RNS_E_INVALID, "a misaligned d_ctl");
    CHECK(rns_tx_tcp_ctl_build_dev(fake, N1, NFLOW, fake, STRIDE, fake, 0, NULL, fake, need, fake, N1, fake, fake, NULL, NULL) ==
              RNS_E_INVALID, "NULL d_count");
    CHECK(rns_tx_tcp_ctl_build_dev(NULL, N1, NFLOW, fake, STRIDE, fake, 0, NULL, fake, need, fake, N1, fake, fake, fake, NULL) ==
              RNS_E_INVALID, "NULL d_ctl");
    CHECK(rns_tx_tcp_ctl_build_dev(fake, N1, NFLOW, fake, 0, fake, 0, NULL, fake, need, fake, N1, fake, fake, fake, NULL) ==
              RNS_E_INVALID, "tmpl_stride 0");
    CHECK(rns_tx_tcp_ctl_build_dev(fake, N1, NFLOW, fake, STRIDE, fake, 0, odd, fake, need, fake, N1, fake, fake, fake, NULL) ==
              RNS_E_INVALID, "a misaligned d_ip_id_add");
    CHECK(rns_tx_tcp_ctl_build_dev(fake, N1, NFLOW, fake, STRIDE, fake, 0, NULL, fake, bneed - 1, fake, N1, fake, fake, fake,
                                   NULL) == RNS_E_INVALID, "a short build workspace");
    CHECK(rns_tx_tcp_ctl_build_dev(fake, N1, NFLOW, fake, STRIDE, fake, 0, NULL, fake, need, NULL, N1, fake, fake, fake, NULL) ==
              RNS_E_INVALID, "NULL d_out with a cap");
    CHECK(rns_tx_tcp_close_dev(NULL, NULL, 0, NULL, NULL, NULL) == RNS_OK, "no flows");
    CHECK(rns_tx_tcp_close_dev(fake, fake, NFLOW, NULL, fake, NULL) == RNS_E_INVALID, "NULL d_op");
    CHECK(rns_tx_tcp_close_dev(fake, fake, NFLOW, fake, NULL, NULL) == RNS_E_INVALID, "NULL d_ctl");
    CHECK(rns_tx_tcp_close_dev(odd, fake, NFLOW, fake, fake, NULL) == RNS_E_INVALID, "a misaligned d_flow_in");
    CHECK(rns_tx_tcp_close_dev(fake, fake, 0x80000000u, fake, fake, NULL) == RNS_E_INVALID, "too many flows");

    rns_rx_tcp_meta *d_b1 = NULL, *d_b2 = NULL;
    rns_tcp_flow *d_f0 = NULL, *d_f1 = NULL, *d_f2 = NULL;
    rns_tcp_ctl *d_c1 = NULL, *d_cc = NULL, *d_c2 = NULL;
    rns_tcp_flow_res *d_res = NULL;
    uint32_t *d_pin = NULL, *d_pout = NULL, *d_src = NULL, *d_n = NULL, *d_add = NULL;
    uint8_t *d_work = NULL, *d_tmpl = NULL, *d_hl = NULL, *d_op = NULL, *d_out = NULL, *d_len = NULL;
    static uint32_t pend[NFLOW * CAP * 2];
    UP(d_b1, b1, sizeof b1);
    UP(d_b2, b2, sizeof b2);
    UP(d_f0, fl, sizeof fl);
    UP(d_pin, pend, sizeof pend);
    UP(d_tmpl, tmpl, sizeof tmpl);
    UP(d_hl, head_len8, sizeof head_len8);
    UP(d_op, op, sizeof op);
    const uint32_t add = 3;
    UP(d_add, &add, sizeof add);
    OUT(d_work, need, FILL);
    OUT(d_f1, sizeof fl, FILL);
    OUT(d_f2, sizeof fl, FILL);
    OUT(d_pout, sizeof pend, FILL);
    OUT(d_c1, N1 * sizeof(rns_tcp_ctl), FILL);
    OUT(d_cc, NFLOW * sizeof(rns_tcp_ctl), FILL);
    OUT(d_c2, N2 * sizeof(rns_tcp_ctl), FILL);
    OUT(d_res, NFLOW * sizeof(rns_tcp_flow_res), FILL);
    OUT(d_out, 64 * NFLOW, FILL);
    OUT(d_src, 4 * NFLOW, FILL);
    OUT(d_len, NFLOW, FILL);
    OUT(d_n, 8, FILL);

    /* one stream of launches: update, close (in place), build over the close records, update */
    CHECK(rns_rx_tcp_conn_update_dev(d_b1, N1, NFLOW, d_f0, d_pin, CAP, d_f1, d_pout, d_c1, d_res, d_work, need, NULL) == RNS_OK,
          "rns_rx_tcp_conn_update_dev");
    rns_tcp_ctl c1[N1], cc[NFLOW], c2[N2];
    rns_tcp_flow f1[NFLOW], f2[NFLOW];
    rns_tcp_flow_res res[NFLOW];
    HIP_OK(hipDeviceSynchronize());
    DOWN(c1, d_c1, sizeof c1);
    DOWN(f1, d_f1, sizeof f1);
    DOWN(res, d_res, sizeof res);
    for (uint32_t i = 0; i < N1; ++i)
        CHECK(c1[i].act == act1[i] && c1[i].flow == b1[i].flow && c1[i].flags == 0 && c1[i].seq == 0, "record %u: act %u != %u",
              i, c1[i].act, act1[i]);
    CHECK(f1[0].state == RNS_TCP_CLOSE_WAIT && f1[0].snd_nxt == 9001 && f1[0].snd_una == 9001 && f1[0].rcv_nxt == 121 &&
              f1[0].rq_len == 20 && f1[0].ack_timer == 1, "flow 0 after the request: state %u", f1[0].state);
    CHECK(memcmp(&f1[1], &fl[1], sizeof fl[1]) == 0 && f1[2].state == RNS_TCP_CLOSED && f1[2].rcv_nxt == 504, "flows 1, 2");
    CHECK(res[0].consumed == 3 && res[0].events == (RNS_EV_WND | RNS_EV_STATE) && res[0].why == RNS_STOP_NONE &&
              res[0].readable == 20 && res[0].n_acks == 0 && res[1].n_segs == 0 && res[2].consumed == 2, "results");

    CHECK(rns_tx_tcp_close_dev(d_f1, d_f1, NFLOW, d_op, d_cc, NULL) == RNS_OK, "rns_tx_tcp_close_dev, in place");
    CHECK(rns_tx_tcp_ctl_build_dev(d_cc, NFLOW, NFLOW, d_tmpl, STRIDE, d_hl, 0xFFFC, d_add, d_work, need, d_out, NFLOW, d_src,
                                   d_len, d_n, NULL) == RNS_OK, "rns_tx_tcp_ctl_build_dev");
    CHECK(rns_rx_tcp_conn_update_dev(d_b2, N2, NFLOW, d_f1, d_pout, CAP, d_f2, d_pin, d_c2, d_res, d_work, need, NULL) == RNS_OK,
          "rns_rx_tcp_conn_update_dev, second batch");
    HIP_OK(hipDeviceSynchronize());
    uint8_t out[64 * NFLOW], len8[NFLOW];
    uint32_t src[NFLOW], cnt[2];
    DOWN(cc, d_cc, sizeof cc);
    DOWN(c2, d_c2, sizeof c2);
    DOWN(f2, d_f2, sizeof f2);
    DOWN(out, d_out, sizeof out);
    DOWN(len8, d_len, sizeof len8);
    DOWN(src, d_src, sizeof src);
    DOWN(cnt, d_n, sizeof cnt);
    const uint8_t fin_act = RNS_CTL_SEND | RNS_CTL_RESP_TIMER | RNS_CTL_STATE;
    /* CloseWait, in order: the FIN is acknowledged (+ 1); Established: never; Closed: no send */
    CHECK(cc[0].act == fin_act && cc[0].flags == 0x11 && cc[0].seq == 9001 && cc[0].ack_num == 122 && cc[0].window == 65515 &&
              cc[0].flow == 0, "close of flow 0: ack %u", cc[0].ack_num);
    CHECK(cc[1].act == fin_act && cc[1].flags == 0x11 && cc[1].seq == 7000 && cc[1].ack_num == 500 && cc[1].window == 65535 &&
              cc[1].flow == 1, "close of flow 1: ack %u", cc[1].ack_num);
    const rns_tcp_ctl zero = {0, 0, 0, 0, 0, 0};
    CHECK(memcmp(&cc[2], &zero, sizeof zero) == 0, "a Closed socket does not send");
    CHECK(cnt[0] == 2 && cnt[1] == 1 && src[0] == 0 && src[1] == 1 && len8[0] == 40 && len8[1] == 60, "counts %u %u", cnt[0], cnt[1]);
    for (uint32_t k = 0; k < 2; ++k) {
        uint8_t h[64];
        const uint32_t hl = ctl_ref(&cc[k], 0xFFFFu, h);   /* 0xfffc + 3: the one IPv4 id */
        CHECK(memcmp(out + 64 * k, h, hl) == 0, "control segment %u: head bytes", k);
        for (uint32_t b = hl; b < 64; ++b)
            CHECK(out[64 * k + b] == FILL, "control segment %u: byte %u of the slot's tail written", k, b);
    }
    for (uint32_t b = 128; b < sizeof out; ++b)
        CHECK(out[b] == FILL, "byte %u past the last segment written", b);
    CHECK(f2[0].state == RNS_TCP_CLOSED && f2[1].state == RNS_TCP_TIME_WAIT && f2[2].state == RNS_TCP_CLOSED, "final states %u %u %u",
          f2[0].state, f2[1].state, f2[2].state);
    CHECK(c2[0].act == (RNS_CTL_CONSUMED | RNS_CTL_STATE) && c2[1].act == (RNS_CTL_CONSUMED | RNS_CTL_STATE), "FinWait2, Closed");
    CHECK(c2[2].act == (RNS_CTL_CONSUMED | RNS_CTL_SEND | RNS_CTL_RESP_TIMER | RNS_CTL_TIMEWAIT | RNS_CTL_STATE) &&
              c2[2].flags == 0x10 && c2[2].seq == 7000 && c2[2].ack_num == 501 && c2[2].flow == 1, "the ACK of the peer's FIN: %u",
          c2[2].ack_num);
    CHECK(f2[0].snd_una == 9001 && f2[1].snd_una == 7000, "the ACK of our FIN trims nothing");

    return abi_finish("%d + %d records of %d flows, %u control segments", N1, N2, NFLOW, cnt[0]);
}
