// stage_layout.hpp -- where the segments of a host entry point sit in the
// context's device scratch (run_items, kite_nmpc.cpp).  Host-only arithmetic,
// no HIP, so that it can be tested without a device (tests/test_stage_layout.py).
//
// A segment is `count` elements of `elem` bytes (8: double, 4: int32_t) with a
// direction.  Segments are laid out in list order, each rounded up to whole
// doubles, so every segment starts 8-byte aligned and none overlap.
//   in       copied host -> device before the launch
//   out      copied device -> host after it
//   inout    both
//   scratch  device only
// A null host pointer copies nothing: an `in` segment is then absent for the
// launch (it sees nullptr; pass the count 0 to reserve nothing), an `out` or
// `inout` segment is a device buffer whose result is not wanted.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace kite_stage {

enum Dir { IN, OUT, INOUT, SCRATCH };

struct Seg {
    void* host;
    size_t count, elem;
    Dir dir;
};

inline Seg in(const double* p, size_t n) { return {const_cast<double*>(p), n, sizeof(double), IN}; }
inline Seg in(const int32_t* p, size_t n) { return {const_cast<int32_t*>(p), n, sizeof(int32_t), IN}; }
inline Seg out(double* p, size_t n) { return {p, n, sizeof(double), OUT}; }
inline Seg out(int32_t* p, size_t n) { return {p, n, sizeof(int32_t), OUT}; }
inline Seg inout(double* p, size_t n) { return {p, n, sizeof(double), INOUT}; }
inline Seg scratch(size_t n) { return {nullptr, n, sizeof(double), SCRATCH}; }

inline size_t doubles(const Seg& s) { return (s.count * s.elem + sizeof(double) - 1) / sizeof(double); }
inline size_t bytes(const Seg& s) { return s.count * s.elem; }
inline bool copies_in(const Seg& s) { return s.host && (s.dir == IN || s.dir == INOUT); }
inline bool copies_out(const Seg& s) { return s.host && (s.dir == OUT || s.dir == INOUT); }
inline bool absent(const Seg& s) { return !s.host && s.dir == IN; }

struct Layout {
    std::vector<size_t> off;     // per segment, in doubles from the start of the scratch
    size_t total = 0;            // doubles
};

inline Layout layout(const std::vector<Seg>& segs) {
    Layout L;
    for (const Seg& s : segs) {
        L.off.push_back(L.total);
        L.total += doubles(s);
    }
    return L;
}

}  // namespace kite_stage
