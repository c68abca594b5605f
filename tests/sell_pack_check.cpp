// Stand-alone check of the host packer of csrc/sell.hpp (tests/test_sell_pack_cpu.py builds it with the address and
// undefined-behaviour sanitizers and runs it): the packed arrays against the layout's naive definition — entry e of the row at
// position p is slot sbase[p / 64] + e * 64 + p % 64 — for the natural order and for level-major positions with empty lanes.
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "sell.hpp"

using sprs::SELL_SLICE;

struct C32 { float re, im; };            // a two-component scalar: T{} must pad with all-zero bits here too

static double make(double, int k) { return k + 1; }
static C32 make(C32, int k) { return C32{(float)(k + 1), -(float)(k + 1)}; }
static bool same(double a, double b) { return a == b; }
static bool same(C32 a, C32 b) { return a.re == b.re && a.im == b.im; }

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAILED %s: %s: ", what, #cond); printf(__VA_ARGS__); printf("\n"); return; } } while (0)

// prow: the row of every position (-1: none); row i has len_of(i) entries in [eb(i), ee(i)), inside a CSR row that is one entry
// longer at either end (so a packer that took the row bounds instead of the range given would be caught)
template <class T>
static void check(const char *what, const std::vector<int32_t> &prow, int nrows, const std::function<int(int)> &len_of) {
    std::vector<int32_t> rp(nrows + 1, 0);
    for (int i = 0; i < nrows; ++i) rp[i + 1] = rp[i] + len_of(i) + 2;
    std::vector<int32_t> ci(rp[nrows]);
    std::vector<T> v(rp[nrows]);
    for (int k = 0; k < rp[nrows]; ++k) { ci[k] = 1 + (k * 7 + 3) % 1000; v[k] = make(T{}, k); }   // no column 0, no zero value
    auto eb = [&](int32_t i) { return rp[i] + 1; };
    auto ee = [&](int32_t i) { return rp[i + 1] - 1; };
    const size_t npos = prow.size();
    const sprs::SellPacked<T> S = sprs::sell_pack<T>((int64_t)npos, [&](size_t p) { return prow[p]; }, eb, ee, ci.data(), v.data());

    const size_t nslice = (npos + SELL_SLICE - 1) / SELL_SLICE;
    CHECK(S.len.size() == nslice * SELL_SLICE && S.sbase.size() == nslice, "%zu lengths, %zu slices", S.len.size(), S.sbase.size());
    int64_t slots = 0;
    for (size_t s = 0; s < nslice; ++s) {
        int width = 0;
        for (size_t p = s * SELL_SLICE; p < (s + 1) * SELL_SLICE; ++p) {
            const int want = p < npos && prow[p] >= 0 ? len_of(prow[p]) : 0;
            CHECK(S.len[p] == want, "len[%zu] = %d, not %d", p, S.len[p], want);
            if (want > width) width = want;
        }
        CHECK(S.sbase[s] == slots, "sbase[%zu] = %lld, not %lld", s, (long long)S.sbase[s], (long long)slots);
        slots += (int64_t)width * SELL_SLICE;
    }
    CHECK(S.slots == slots && S.col.size() == (size_t)slots && S.val.size() == (size_t)slots, "%lld slots, not %lld", (long long)S.slots, (long long)slots);
    std::vector<char> used((size_t)slots, 0);
    for (size_t p = 0; p < npos; ++p) {
        if (prow[p] < 0) continue;
        for (int e = 0; e < len_of(prow[p]); ++e) {
            const size_t d = (size_t)S.sbase[p / SELL_SLICE] + (size_t)e * SELL_SLICE + p % SELL_SLICE, k = (size_t)eb(prow[p]) + e;
            CHECK(d < (size_t)slots && !used[d], "entry %d of position %zu: slot %zu", e, p, d);
            used[d] = 1;
            CHECK(S.col[d] == ci[k] && same(S.val[d], v[k]), "entry %d of position %zu holds column %d", e, p, S.col[d]);
        }
    }
    const T zero{};
    for (size_t d = 0; d < (size_t)slots; ++d)
        CHECK(used[d] || (S.col[d] == 0 && memcmp(&S.val[d], &zero, sizeof(T)) == 0), "padded slot %zu holds column %d", d, S.col[d]);
}

template <class T>
static void all_cases() {
    char what[96];
    auto cyc = [](int i) { return i % 10; };                 // lengths 0 .. 9: every remainder of the fold's unroll by four
    for (int n : {0, 1, 63, 64, 65, 129}) {
        std::vector<int32_t> prow(n);
        for (int i = 0; i < n; ++i) prow[i] = i;
        snprintf(what, sizeof(what), "natural n = %d, %zu-byte scalars", n, sizeof(T));
        check<T>(what, prow, n, cyc);
    }
    {   // the middle slice of three holds empty rows only
        std::vector<int32_t> prow(129);
        for (int i = 0; i < 129; ++i) prow[i] = i;
        snprintf(what, sizeof(what), "natural n = 129 with an empty slice, %zu-byte scalars", sizeof(T));
        check<T>(what, prow, 129, [](int i) { return i >= 64 && i < 128 ? 0 : i % 10; });
    }
    {   // level-major: levels of 1, 64 and 65 rows -> 1 + 1 + 2 slices, the first and the last part-filled; rows in scrambled order
        const int nrows = 130, sizes[3] = {1, 64, 65};
        std::vector<int32_t> prow;
        int r = 0;
        for (int sz : sizes) {
            for (int k = 0; k < sz; ++k, ++r) prow.push_back((r * 37) % nrows);   // 37 and 130 are coprime: a permutation
            prow.resize((prow.size() + SELL_SLICE - 1) / SELL_SLICE * SELL_SLICE, -1);
        }
        snprintf(what, sizeof(what), "level-major 1 + 64 + 65 rows, %zu-byte scalars", sizeof(T));
        check<T>(what, prow, nrows, cyc);
        if (prow.size() != 4 * SELL_SLICE) { ++failures; printf("FAILED %s: %zu positions\n", what, prow.size()); }
    }
}

int main() {
    all_cases<double>();
    all_cases<C32>();
    printf(failures ? "%d case(s) failed\n" : "sell_pack: all cases passed\n", failures);
    return failures ? 1 : 0;
}
