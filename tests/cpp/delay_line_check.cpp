// delay_line_check -- the command line's host-compilable functions
// (openkite_amd/csrc/delay_line.hpp: delay_send, inflight_row,
// inflight_substeps) against tables written by the Python models
// (tools/delay_line_tables.py from tests/delay_rule_ref.py).  A stand-alone
// host program, meant to be built with the sanitizers and run on the CPU:
//
//   python tools/delay_line_tables.py tables.txt
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Iopenkite_amd/csrc tests/cpp/delay_line_check.cpp -o delay_line_check
//   ./delay_line_check tables.txt
//
// Table lines (doubles as C99 hex floats, "nan", "inf"):
//   send  <32 line> <4 u_cmd> <tau> <t0> <has_cmd>  ->  <32 line> <n> <flag>   (the count slot: see below)
//   row   <32 line> <t0>                            ->  <24 schedule row>
//   sub   <len> <h_max> <steps>                     ->  <n>
// Every comparison is bitwise (NaN equals NaN).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "delay_line.hpp"

namespace {

bool same(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0 || (a != a && b != b); }

bool read_doubles(std::istringstream& in, int n, std::vector<double>& out) {
    out.clear();
    std::string tok;
    for (int i = 0; i < n; ++i) {
        if (!(in >> tok)) return false;
        out.push_back(std::strtod(tok.c_str(), nullptr));
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s tables.txt\n", argv[0]); return 2; }
    std::ifstream f(argv[1]);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string ln;
    long nsend = 0, nrow = 0, nsub = 0, bad = 0, lineno = 0;
    while (std::getline(f, ln)) {
        ++lineno;
        if (ln.empty() || ln[0] == '#') continue;
        std::istringstream in(ln);
        std::string kind;
        in >> kind;
        std::vector<double> a, b;
        if (kind == "send") {
            if (!read_doubles(in, KITE_DELAY_NLINE + 4 + 3, a) || !read_doubles(in, KITE_DELAY_NLINE + 2, b)) return 3;
            // heap copies of exactly the sizes the functions may touch: an overrun is the sanitizer's
            std::vector<double> L(a.begin(), a.begin() + KITE_DELAY_NLINE);
            std::vector<double> u(a.begin() + KITE_DELAY_NLINE, a.begin() + KITE_DELAY_NLINE + 4);
            std::vector<double> tau(1, a[KITE_DELAY_NLINE + 4]);
            const double t0 = a[KITE_DELAY_NLINE + 5];
            const bool has = a[KITE_DELAY_NLINE + 6] != 0.0;
            int32_t flag = 0;
            const int n = kite::delay_send(L.data(), has ? u.data() : nullptr, has ? tau.data() : nullptr, 0, t0, flag);
            bool ok = n == (int)b[KITE_DELAY_NLINE] && flag == (int32_t)b[KITE_DELAY_NLINE + 1];
            // the send returns the count; the slot is written when the call ends (delay_finish)
            for (int j = 0; j < KITE_DELAY_NLINE; ++j) ok = ok && (j == KITE_DELAY_COUNT ? same(L[j], a[j]) : same(L[j], b[j]));
            if (!ok && ++bad <= 10) std::fprintf(stderr, "line %ld: send differs (n %d, flag %d)\n", lineno, n, (int)flag);
            ++nsend;
        } else if (kind == "row") {
            if (!read_doubles(in, KITE_DELAY_NLINE + 1, a) || !read_doubles(in, KITE_INFLIGHT_N, b)) return 3;
            std::vector<double> L(a.begin(), a.begin() + KITE_DELAY_NLINE), row(KITE_INFLIGHT_N, 777.0);
            kite::inflight_row(L.data(), a[KITE_DELAY_NLINE], row.data());
            bool ok = true;
            for (int j = 0; j < KITE_INFLIGHT_N; ++j) ok = ok && same(row[j], b[j]);
            if (!ok && ++bad <= 10) std::fprintf(stderr, "line %ld: schedule row differs\n", lineno);
            ++nrow;
        } else if (kind == "sub") {
            if (!read_doubles(in, 3, a) || !read_doubles(in, 1, b)) return 3;
            const int n = kite::inflight_substeps(a[0], a[1], (int)a[2]);
            if (n != (int)b[0] && ++bad <= 10) std::fprintf(stderr, "line %ld: substeps %d, table %d\n", lineno, n, (int)b[0]);
            ++nsub;
        } else {
            std::fprintf(stderr, "line %ld: unknown record %s\n", lineno, kind.c_str());
            return 3;
        }
    }
    std::printf("delay_line_check: %ld sends, %ld schedule rows, %ld substep counts, %ld differ\n", nsend, nrow, nsub, bad);
    return bad ? 1 : 0;
}
