// Stand-alone check of openkite_amd/csrc/stage_layout.hpp (tests/test_stage_layout.py
// builds it with -fsanitize=address,undefined and runs it).  The segment lists are the
// ones kite_nmpc.cpp passes to run_items; the expected offsets and totals (in doubles)
// are written out from the arithmetic those entry points carved their scratch with
// before they shared run_items.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "stage_layout.hpp"

namespace ks = kite_stage;

static int failures = 0;

static void expect(const char* what, const std::vector<ks::Seg>& segs, const std::vector<size_t>& off, size_t total) {
    const ks::Layout L = ks::layout(segs);
    bool ok = L.off == off && L.total == total;
    // every segment starts on a whole double and ends before the next one starts
    std::vector<double> arena(L.total + 1);
    for (size_t i = 0; i < segs.size(); ++i) {
        const char* lo = reinterpret_cast<const char*>(arena.data() + L.off[i]);
        const char* hi = lo + ks::bytes(segs[i]);
        ok = ok && reinterpret_cast<uintptr_t>(lo) % 8 == 0;
        const char* next = reinterpret_cast<const char*>(arena.data() + (i + 1 < segs.size() ? L.off[i + 1] : L.total));
        ok = ok && hi <= next;
    }
    if (!ok) {
        ++failures;
        std::printf("FAIL %s: total %zu (want %zu), offsets", what, L.total, total);
        for (size_t o : L.off) std::printf(" %zu", o);
        std::printf("\n");
    }
}

static void check(const char* what, bool ok) {
    if (!ok) { ++failures; std::printf("FAIL %s\n", what); }
}

// kite_nmpc_windekf_step
static std::vector<ks::Seg> windekf(size_t c, bool with_z, bool with_status) {
    static double x[16 * 5], u[3 * 5], P[256 * 5], z[7 * 5], W[256], V[49];
    static int32_t st[5];
    const double* z7 = with_z ? z : nullptr;
    return {ks::inout(x, c * 16), ks::in(u, c * 3), ks::inout(P, c * 256), ks::in(z7, z7 ? c * 7 : 0),
            ks::in(W, 256), ks::in(V, 49), ks::out(with_status ? st : nullptr, c)};
}

int main() {
    for (int with_status = 0; with_status < 2; ++with_status) {
        // x16 | u3 | P256 | z7 | W256 | V49 | status: (16 + 3 + 256 + 7) c + 256 + 49 + (c + 1) / 2
        expect("windekf c=1 z", windekf(1, true, with_status), {0, 16, 19, 275, 282, 538, 587}, 588);
        expect("windekf c=5 z", windekf(5, true, with_status), {0, 80, 95, 1375, 1410, 1666, 1715}, 1718);
        // no measurement: z7 reserves nothing
        expect("windekf c=1", windekf(1, false, with_status), {0, 16, 19, 275, 275, 531, 580}, 581);
        expect("windekf c=5", windekf(5, false, with_status), {0, 80, 95, 1375, 1375, 1631, 1680}, 1683);
        const std::vector<ks::Seg> s = windekf(5, false, with_status);
        check("windekf: no z is absent", ks::absent(s[3]) && !ks::copies_in(s[3]));
        check("windekf: status copy-out follows the pointer", ks::copies_out(s[6]) == (with_status != 0));
        check("windekf: a status buffer either way", !ks::absent(s[6]));
        check("windekf: x goes both ways", ks::copies_in(s[0]) && ks::copies_out(s[0]));
        check("windekf: u goes in only", ks::copies_in(s[1]) && !ks::copies_out(s[1]));
    }
    {   // kite_nmpc_plant_step_delayed, B = 5, without a command: the slots of
        // u4_cmd and tau stay (x13 | u4_cmd | tau | line | u4_applied | status)
        static double x[65], line[160], ua[20];
        static int32_t st[5];
        const double *u4_cmd = nullptr, *tau = nullptr;
        const size_t B = 5;
        const std::vector<ks::Seg> s = {ks::inout(x, B * 13), ks::in(u4_cmd, B * 4), ks::in(u4_cmd ? tau : nullptr, B),
                                        ks::inout(line, B * 32), ks::out(ua, B * 4), ks::out(st, B)};
        expect("plant_step_delayed B=5 no command", s, {0, 65, 85, 90, 250, 270}, 273);
        check("plant_step_delayed: no command, no latencies", ks::absent(s[1]) && ks::absent(s[2]));
        check("plant_step_delayed: the line goes both ways", ks::copies_in(s[3]) && ks::copies_out(s[3]));
    }
    {   // kite_nmpc_score_step, c = 5, without the plant's status words
        // (x13 | u4 | acc16 | mem8 | status | plant_status)
        static double x[65], u[20], acc[80], mem[40];
        static int32_t st[5];
        const int32_t* ps = nullptr;
        const size_t c = 5;
        const std::vector<ks::Seg> s = {ks::in(x, c * 13), ks::in(u, c * 4), ks::inout(acc, c * 16),
                                        ks::inout(mem, c * 8), ks::in(st, c), ks::in(ps, c)};
        expect("score_step c=5", s, {0, 65, 85, 165, 205, 208}, 211);
        check("score_step: status in, plant_status absent", ks::copies_in(s[4]) && ks::absent(s[5]));
    }
    // an odd int32 count rounds up to whole doubles, an even one does not grow
    check("int32 x 5 is 3 doubles", ks::doubles(ks::out(static_cast<int32_t*>(nullptr), 5)) == 3);
    check("int32 x 4 is 2 doubles", ks::doubles(ks::out(static_cast<int32_t*>(nullptr), 4)) == 2);
    check("int32 x 1 is 1 double", ks::doubles(ks::in(static_cast<const int32_t*>(nullptr), 1)) == 1);
    check("scratch copies nothing", !ks::copies_in(ks::scratch(7)) && !ks::copies_out(ks::scratch(7)) &&
                                        !ks::absent(ks::scratch(7)));
    std::printf(failures ? "%d failure(s)\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
