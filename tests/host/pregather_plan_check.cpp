// Walks the slice planner of k_wgrad_adam's riders (mamdr_amd/csrc/pregather_plan.h) over every pass-size list of up to four
// passes: every row and every padding row is handed out exactly once, no slice has more than two segments or more than its
// quota, a segment stays inside its pass, and the cursor ends behind the last pass.  Built and run by
// tests/test_pregather_plan_host.py with the host compiler's address and undefined-behaviour sanitizers.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pregather_plan.h"

using namespace mamdr;

static int fails = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (fails++ < 20) {                           \
                std::printf("FAIL %s: ", #cond);          \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

static long walk(const std::vector<int64_t>& rows, int64_t quota) {
    const int n = (int)rows.size();
    std::vector<std::vector<int>> seen(n);
    int64_t total = 0;
    for (int k = 0; k < n; ++k) {
        seen[k].assign((size_t)pre_plan_positions(rows[k]), 0);
        total += pre_plan_positions(rows[k]);
    }
    PrePlanCursor cur;
    long slices = 0;
    int64_t got = 0;
    for (;;) {
        const PrePlanSlice s = pre_plan_next(rows.data(), n, cur, quota);
        if (s.count() == 0) break;
        ++slices;
        CHECK(slices <= total + 1, "planner does not terminate (quota %lld)", (long long)quota);
        if (slices > total + 1) break;
        CHECK(s.n_seg >= 1 && s.n_seg <= 2, "n_seg %d", s.n_seg);
        CHECK(s.count() <= quota, "slice of %lld positions, quota %lld", (long long)s.count(), (long long)quota);
        for (int g = 0; g < s.n_seg && g < 2; ++g) {
            const PrePlanSeg& q = s.seg[g];
            CHECK(q.pass >= 0 && q.pass < n, "pass %d of %d", q.pass, n);
            if (q.pass < 0 || q.pass >= n) continue;
            CHECK(q.count > 0 && q.first >= 0 && q.first + q.count <= pre_plan_positions(rows[q.pass]),
                  "segment [%lld, +%lld) of a pass of %lld rows", (long long)q.first, (long long)q.count, (long long)rows[q.pass]);
            if (g == 1) CHECK(q.pass > s.seg[0].pass && q.first == 0, "second segment does not open a later pass");
            for (int64_t i = q.first; i < q.first + q.count && i < (int64_t)seen[q.pass].size(); ++i) seen[q.pass][(size_t)i] += 1;
            got += q.count;
        }
        if (s.n_seg < 2) CHECK(s.seg[1].count == 0, "unused segment carries %lld positions", (long long)s.seg[1].count);
    }
    CHECK(got == total, "%lld of %lld positions handed out", (long long)got, (long long)total);
    for (int k = 0; k < n; ++k)
        for (size_t i = 0; i < seen[k].size(); ++i)
            CHECK(seen[k][i] == 1, "position %zu of pass %d (%lld rows) handed out %d times, quota %lld", i, k, (long long)rows[k],
                  seen[k][i], (long long)quota);
    CHECK(cur.pass == n && cur.pos == 0, "cursor ends at (%d, %lld) of %d passes", cur.pass, (long long)cur.pos, n);
    // ... and stays there
    const PrePlanSlice again = pre_plan_next(rows.data(), n, cur, quota);
    CHECK(again.n_seg == 0 && again.count() == 0 && cur.pass == n, "a finished window hands out more");
    return slices;
}

int main() {
    const int64_t sizes[] = {0, 1, 15, 16, 17, 1025}, quotas[] = {1, 64, 896};
    long lists = 0, slices = 0;
    for (int len = 0; len <= 4; ++len) {
        int combos = 1;
        for (int k = 0; k < len; ++k) combos *= 6;
        for (int c = 0; c < combos; ++c) {
            std::vector<int64_t> rows;
            for (int k = 0, r = c; k < len; ++k, r /= 6) rows.push_back(sizes[r % 6]);
            for (int64_t q : quotas) slices += walk(rows, q);
            ++lists;
        }
    }
    std::printf("%ld pass lists, %ld slices, %d failures\n", lists, slices, fails);
    return fails ? 1 : 0;
}
