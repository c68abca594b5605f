// The host part of csrc/bjacobi_plan.hpp against the naive definition of the layout: rows are dealt to the lanes of 64-lane slices
// block after block, a block that does not fit what is left of a slice starting the next.  Stand-alone (the standard library and
// the header's host part only); tests/test_bjacobi_plan_cpu.py builds it with the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "bjacobi_plan.hpp"

using namespace sprs;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static std::vector<int64_t> ptr_of(const std::vector<int> &sizes) {
    std::vector<int64_t> bp{0};
    for (int m : sizes) bp.push_back(bp.back() + m);
    return bp;
}

static void check_layout(const char *name, const std::vector<int> &sizes, int64_t want_slices) {
    const std::vector<int64_t> bp = ptr_of(sizes);
    const BjacobiPlan P = bjacobi_plan(bp);
    // ---- the naive layout: (slice, lane) of every row, per slice its first row, rows and width
    struct Row { int64_t slice; int lane, first, m; int64_t block; };
    std::vector<Row> rows;
    std::vector<int64_t> first_row, cnt, width;
    int lane = BJ_SLICE;
    for (size_t b = 0; b < sizes.size(); ++b) {
        const int m = sizes[b];
        if (lane + m > BJ_SLICE) { first_row.push_back(bp[b]); cnt.push_back(0); width.push_back(0); lane = 0; }
        for (int i = 0; i < m; ++i) rows.push_back(Row{(int64_t)first_row.size() - 1, lane + i, lane, m, (int64_t)b});
        cnt.back() += m; if (width.back() < m) width.back() = m;
        lane += m;
    }
    const int64_t n = bp.back(), nslice = (int64_t)first_row.size();
    CHECK(P.fits, "%s: the layout is said not to fit 32-bit positions", name);
    CHECK(P.n == n && P.nblocks == (int64_t)sizes.size(), "%s: n %lld nblocks %lld", name, (long long)P.n, (long long)P.nblocks);
    CHECK(P.nslice() == nslice && nslice == want_slices, "%s: %lld slices, naive %lld, expected %lld", name, (long long)P.nslice(), (long long)nslice, (long long)want_slices);
    if (P.nslice() != nslice) return;
    CHECK(P.scnt.size() == (size_t)nslice && P.sbase.size() == (size_t)nslice && P.code.size() == (size_t)nslice * BJ_SLICE && P.bpos.size() == sizes.size(), "%s: array sizes", name);
    int64_t slots = 0, maxb = 0;
    for (int64_t s = 0; s < nslice; ++s) {
        CHECK(P.srow[s] == first_row[s] && P.scnt[s] == cnt[s], "%s: slice %lld rows %d + %d", name, (long long)s, P.srow[s], P.scnt[s]);
        CHECK(P.scnt[s] >= 1 && P.scnt[s] <= BJ_SLICE, "%s: slice %lld holds %d rows", name, (long long)s, P.scnt[s]);
        CHECK(P.sbase[s] == slots, "%s: slice %lld base %lld, naive %lld", name, (long long)s, (long long)P.sbase[s], (long long)slots);
        slots += width[s] * BJ_SLICE;
    }
    for (int m : sizes) if (m > maxb) maxb = m;
    CHECK(P.slots == slots && P.max_block == maxb, "%s: slots %lld (naive %lld) max_block %lld", name, (long long)P.slots, (long long)slots, (long long)P.max_block);
    // ---- per position: the code of the row that sits there, 0 where none does; rows in natural order from lane 0
    std::vector<uint16_t> code((size_t)nslice * BJ_SLICE, 0);
    for (int64_t r = 0; r < n; ++r) {
        const Row &w = rows[(size_t)r];
        code[(size_t)(w.slice * BJ_SLICE + w.lane)] = (uint16_t)(w.first | (w.m << 8));
        CHECK(P.srow[w.slice] + w.lane == r, "%s: row %lld is not at lane %d of slice %lld", name, (long long)r, w.lane, (long long)w.slice);
        CHECK(w.first + w.m <= BJ_SLICE, "%s: block %lld straddles a slice", name, (long long)w.block);
    }
    CHECK(code == P.code, "%s: position codes", name);
    // ---- every entry's slot: the formula, inside the slice's extent, no slot twice
    std::set<int64_t> seen;
    int64_t r = 0;
    for (size_t b = 0; b < sizes.size(); ++b) {
        const int m = sizes[b];
        CHECK(P.bpos[b] == rows[(size_t)r].slice * BJ_SLICE + rows[(size_t)r].lane, "%s: block %zu position %d", name, b, P.bpos[b]);
        for (int i = 0; i < m; ++i, ++r) {
            const Row &w = rows[(size_t)r];
            for (int j = 0; j < m; ++j) {
                const int64_t want = P.sbase[w.slice] + (int64_t)j * BJ_SLICE + w.lane, got = P.slot((int64_t)b, i, j);
                CHECK(got == want, "%s: slot of (%zu, %d, %d) is %lld, naive %lld", name, b, i, j, (long long)got, (long long)want);
                CHECK(got >= P.sbase[w.slice] && got < P.sbase[w.slice] + width[w.slice] * BJ_SLICE && got < P.slots, "%s: slot %lld outside its slice", name, (long long)got);
                CHECK(seen.insert(got).second, "%s: slot %lld twice", name, (long long)got);
            }
        }
    }
    std::printf("%-28s rows %5lld blocks %4zu slices %3lld slots %6lld\n", name, (long long)n, sizes.size(), (long long)nslice, (long long)slots);
}

static std::vector<int> uniform(int64_t n, int bs) {
    std::vector<int64_t> bp;
    int64_t at = -7;
    const int st = bjacobi_block_ptr(n, bs, nullptr, 0, bp, &at);
    CHECK(st == 0 && at == -1 && bp.front() == 0 && bp.back() == n, "uniform(%lld, %d): status %d", (long long)n, bs, st);
    std::vector<int> sizes;
    for (size_t b = 0; b + 1 < bp.size(); ++b) {
        sizes.push_back((int)(bp[b + 1] - bp[b]));
        CHECK(sizes.back() == bs || (b + 2 == bp.size() && sizes.back() >= 1 && sizes.back() < bs), "uniform(%lld, %d): block %zu has %d rows", (long long)n, bs, b, sizes.back());
    }
    return sizes;
}

int main() {
    check_layout("n = 1", uniform(1, 1), 1);
    check_layout("n = 1, bs = 32", uniform(1, 32), 1);
    check_layout("bs = 1, n = 130", uniform(130, 1), 3);
    check_layout("bs = 3, n = 200 (ragged)", uniform(200, 3), 4);          // 21 blocks = 63 lanes a slice: 63, 63, 63, 11
    check_layout("bs = 32, n = 128", uniform(128, 32), 2);
    check_layout("bs = 32, n = 150 (ragged)", uniform(150, 32), 3);        // 64, 64, 22
    check_layout("bs = 17, n = 100", uniform(100, 17), 2);            // 17 * 3 = 51, then 17 * 2 + 15
    check_layout("bs = 5, n = 64", uniform(64, 5), 1);                     // 12 blocks = 60 lanes, and the ragged 4 fill the slice
    check_layout("bs = 5, n = 65", uniform(65, 5), 2);                     // 13 blocks: the last does not fit
    {
        std::vector<int> cyc;
        for (int rep = 0; rep < 3; ++rep) for (int m = 1; m <= 32; ++m) cyc.push_back(m);
        check_layout("sizes cycling 1 .. 32", cyc, 30);
    }
    check_layout("a slice filled to exactly 64", {32, 16, 8, 8, 5}, 2);
    check_layout("exactly 64 twice", {31, 33 - 1, 1, 20, 20, 24}, 2);
    check_layout("a block that would straddle", {30, 30, 5, 30, 4, 1}, 2);  // 60 lanes, the 5 opens the next slice: 5 + 30 + 4 + 1
    check_layout("straddle by one", {32, 31, 2, 1}, 2);                    // 63 lanes, the 2 does not fit
    check_layout("no blocks", {}, 0);
    // ---- bjacobi_block_ptr's refusals
    std::vector<int64_t> bp;
    int64_t at = -7;
    const int64_t good[] = {0, 3, 4, 36}, not0[] = {1, 3, 4, 36}, flat[] = {0, 3, 3, 36}, back[] = {0, 5, 4, 36}, big[] = {0, 3, 36, 70};
    CHECK(bjacobi_block_ptr(36, 0, good, 3, bp, &at) == 0 && bp.size() == 4 && bp[2] == 4, "a good block_ptr");
    CHECK(bjacobi_block_ptr(36, 0, not0, 3, bp, &at) == 1, "does not start at 0");
    CHECK(bjacobi_block_ptr(36, 0, flat, 3, bp, &at) == 2 && at == 1, "an empty block");
    CHECK(bjacobi_block_ptr(36, 0, back, 3, bp, &at) == 2 && at == 1, "a decreasing block_ptr");
    CHECK(bjacobi_block_ptr(37, 0, good, 3, bp, &at) == 3, "does not end at n");
    CHECK(bjacobi_block_ptr(70, 0, big, 3, bp, &at) == 4 && at == 1, "a block of 33");
    CHECK(bjacobi_block_ptr(70, 33, nullptr, 0, bp, &at) == 4, "block_size 33");
    CHECK(bjacobi_block_ptr(36, 0, good, -1, bp, &at) == 1, "negative nblocks");
    const int64_t zero[] = {0};
    CHECK(bjacobi_block_ptr(0, 0, zero, 0, bp, &at) == 0 && bp.size() == 1, "no rows");
    CHECK(bjacobi_block_ptr(0, 4, nullptr, 0, bp, &at) == 0 && bp.size() == 1, "no rows, uniform");
    std::printf(failures ? "%d FAILURES\n" : "all layouts match\n", failures);
    return failures ? 1 : 0;
}
