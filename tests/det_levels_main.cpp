// Stand-alone check of the level plan of kge_segment_sum_ordered (torchkge_amd/csrc/segment_levels.h): host arithmetic
// only.  tests/test_deterministic_host.py compiles it with -fsanitize=address,undefined and runs it.  For every M it
// walks the plan exactly as the launcher and the kernel index it -- every slot key and slot row a level writes must lie
// inside the workspace the plan sized, and inside the next level's range -- by touching a real buffer of that size.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../torchkge_amd/csrc/segment_levels.h"

static int fail(const char *what, long long M, int d)
{
    std::fprintf(stderr, "FAIL %s at M = %lld, d = %d\n", what, M, d);
    return 1;
}

static int check(int64_t M, int d, bool touch)
{
    const kge_det_plan p = kge_det_make_plan(M, d);
    if (M <= 0 || M > KGE_DET_MAX_M || d < 1 || d > 1024) return (p.n_levels == 0 && p.bytes == 0) ? 0 : fail("refusal", M, d);
    if (p.n_levels < 1 || p.n_levels > KGE_DET_MAX_LEVELS || p.bytes < 16 || p.m[0] != M) return fail("plan", M, d);
    int64_t slots = 0;
    for (int l = 0; l < p.n_levels; ++l) {
        const int64_t chunks = (p.m[l] + KGE_DET_CH - 1) / KGE_DET_CH;
        const bool last = l == p.n_levels - 1;
        if (last != (chunks == 1)) return fail("last level", M, d);
        if (l) {
            if (p.key_off[l] != slots || p.row_off[l] != slots) return fail("offsets", M, d);
            slots += p.m[l];
        }
        if (!last && p.m[l + 1] != 2 * chunks) return fail("next level", M, d);
    }
    if (slots != p.slots) return fail("slot count", M, d);
    if ((unsigned long long)p.slots * (8ull + 4ull * d) > p.bytes) return fail("bytes", M, d);
    if (!touch) return 0;
    std::vector<unsigned char> ws(p.bytes);
    int64_t *keys = reinterpret_cast<int64_t *>(ws.data());
    float *rows = reinterpret_cast<float *>(keys + p.slots);
    for (int l = 0; l + 1 < p.n_levels; ++l) {
        const int64_t chunks = (p.m[l] + KGE_DET_CH - 1) / KGE_DET_CH;
        int64_t *sk = keys + p.key_off[l + 1];
        float *sr = rows + p.row_off[l + 1] * d;
        for (int64_t c = 0; c < chunks; ++c)
            for (int s = 0; s < 2; ++s) {
                sk[2 * c + s] = c;                                          // what store_slot writes
                std::memset(sr + (2 * c + s) * d, 0, sizeof(float) * d);
            }
    }
    return 0;
}

int main()
{
    int bad = 0;
    const int ds[] = {1, 63, 64, 200, 1024};
    for (int d : ds)
        for (int64_t M = -1; M <= 5000; ++M) bad += check(M, d, (d == 1 || d == 200) && M <= 2200);
    for (int64_t M : {65536ll, 65537ll, 1048576ll}) bad += check(M, 3, true);
    bad += check(4194304, 512, false) + check(KGE_DET_MAX_M, 1024, false) + check(KGE_DET_MAX_M, 1, false);
    bad += check(KGE_DET_MAX_M + 1, 1, false) + check(INT64_MAX, 1024, false) + check(INT64_MAX, 1, false);
    bad += check(5, 0, false) + check(5, 1025, false);
    // monotone in M and in d, 0 only at M <= 0
    size_t prev = 0;
    for (int64_t M = 0; M <= 70000; ++M) {
        const size_t b = kge_det_make_plan(M, 200).bytes;
        if (b < prev || (M > 0) != (b > 0)) bad += fail("monotone in M", M, 200);
        prev = b;
    }
    for (int64_t M : {1ll, 33ll, 2053ll, 65536ll}) {
        prev = 0;
        for (int d = 1; d <= 1024; ++d) {
            const size_t b = kge_det_make_plan(M, d).bytes;
            if (b < prev) bad += fail("monotone in d", M, d);
            prev = b;
        }
    }
    const kge_det_plan p = kge_det_make_plan(2053, 8);
    if (p.n_levels != 3 || p.m[1] != 130 || p.m[2] != 10) bad += fail("2053 -> 130 -> 10", 2053, 8);
    if (kge_det_make_plan(4194304, 8).n_levels != 6) bad += fail("levels at 4 M", 4194304, 8);
    std::printf(bad ? "level plan: %d failures\n" : "level plan: ok\n", bad);
    return bad ? 1 : 0;
}
