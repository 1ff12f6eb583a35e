// The connection update's step (conn_step, conn_stop_first, conn_close of rns_k_conn.hpp) compiled by a host
// compiler: the same RNS_HD functions the device's walks run, over a table of one-segment cases read from a
// file, the results written to another.  tests/test_conn_step.py writes the table, builds this program twice
// (once with -fsanitize=address,undefined) and compares the results with tests/tcp_conn_helper.py.
//
// A case, one line of unsigned decimals:   op f0 .. f9 seq ack win_pay misc pend_cap p0 .. p(2 * pend_cap - 1)
//   op 0: one segment through conn_stop_first and conn_step;  op 1: conn_close (the segment's fields unused).
// Its result, one line:   why f0 .. f9 readable acked n_acks events c0 c1 c2 c3 p0 .. p(2 * n_pend - 1)
//   c = the rns_tcp_ctl record's four dwords for flow 7 (zero when the segment is not consumed).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rns_k_conn.hpp"

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s table results\n", argv[0]);
        return 2;
    }
    std::FILE *in = std::fopen(argv[1], "r"), *out = std::fopen(argv[2], "w");
    if (!in || !out) {
        std::fprintf(stderr, "cannot open the files\n");
        return 2;
    }
    unsigned long n = 0;
    unsigned op;
    while (std::fscanf(in, "%u", &op) == 1) {
        uint32_t r[10], seg[4], cap;
        for (uint32_t &x : r)
            if (std::fscanf(in, "%u", &x) != 1)
                return 3;
        for (uint32_t &x : seg)
            if (std::fscanf(in, "%u", &x) != 1)
                return 3;
        if (std::fscanf(in, "%u", &cap) != 1 || cap > 64)
            return 3;
        std::vector<uint32_t> pend(2 * cap);  // exactly the flow's range: a write past it is the sanitizer's to see
        for (uint32_t &x : pend)
            if (std::fscanf(in, "%u", &x) != 1)
                return 3;
        rns::FlowState s;
        rns::flow_load(s, r);
        uint32_t why = rns::kStopNone, ctl[4] = {0, 0, 0, 0};
        const uint32_t f = 7;
        if (op == 0) {
            uint32_t ack_num = 0, seq_out = 0, last = 0;
            why = rns::ConnStepOp::first(s, 1, cap);
            if (why == rns::kStopNone)
                why = rns::ConnStepOp::step(s, pend.data(), cap, seg[0], seg[1], seg[2], seg[3], ack_num, seq_out, last);
            if (why == rns::kStopNone) {
                ctl[0] = f;
                ctl[1] = seq_out;
                ctl[2] = ack_num;
                ctl[3] = last;
            }
        } else {
            rns::conn_close(s, f, ctl);
        }
        uint32_t w[10];
        rns::flow_store(s, w);
        std::fprintf(out, "%u", why);
        for (uint32_t x : w)
            std::fprintf(out, " %u", x);
        std::fprintf(out, " %u %u %u %u %u %u %u %u", s.readable, s.acked, s.n_acks, s.events, ctl[0], ctl[1], ctl[2], ctl[3]);
        for (uint32_t k = 0; k < 2 * s.n_pend && k < 2 * cap; ++k)
            std::fprintf(out, " %u", pend[k]);
        std::fprintf(out, "\n");
        ++n;
    }
    std::fclose(in);
    if (std::fclose(out) != 0)
        return 2;
    std::printf("%lu cases\n", n);
    return 0;
}
