// check_pass_budget.cpp -- a stand-alone check of the pass-size rule (csrc/pass_budget.h: pass_size_for) on the CPU. The rule is what pt_render, pt_ao_render and
// pt_aov_render choose a pass by when the caller leaves spp_per_pass = 0; it makes no HIP call, so this program needs no device. It exits 0 when every check holds.
//
// For every combination of: 256 pixel slots, 1..7 samples, a workspace of 256 + 4 x 13 and 256 + 4 x 31 bytes per path (an ordinary scene's queues and the most a scene can
// have), the budgets of the three integrators (path: no extra bytes, 0.65, 2^29 paths; feature buffers: 32 bytes, 0.5; AO: 4 + K x 40 bytes, 0.5, 2^31 / K paths at K = 1
// and K = 64) and two caps small enough to bind, share 1 and 2, free memory from 0 across every boundary between s and s + 1 affordable samples, and a present workspace of
// 0, 2 and 5 samples -- the chosen S
//   * is at least 1 and at most the samples asked for, and makes passes of equal size: ceil(n / ceil(n / S)) == S;
//   * needs no more than fraction x (free / share + held) bytes at per_path -- unless it is the floor of one sample per pass, which a render cannot go below, or fits what the
//     present workspace already holds (a workspace that exists is affordable: the path integrator's rule since the workspace became persistent);
//   * keeps pixel slots x S within the cap / share (again but for the floor);
//   * is not smaller than it has to be: S + 1 would break the memory bound or the cap, or S already is n, or the equal-pass rounding brought it down from such a size;
//   * for a budget without extra bytes, is what the path integrator's former formula chose (restated below): pt_render's choice does not move.
// n_pix_slots == 0, free == 0, share == 0 and n_samples == 0 must not divide by zero.
#include "pass_budget.h"
#include <cstdio>
#include <initializer_list>
#include <vector>

using namespace pth;

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_failed <= 20) { std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// choose_pass_size as it stood before the rule moved to pass_budget.h (capacity = paths the present workspace holds)
static uint32_t former_path_rule(size_t free_b, size_t capacity, size_t per_path, uint32_t n_pix_slots, uint32_t spp, uint32_t share) {
    const size_t kPassMaxPaths = (size_t)1 << 29; const double kPassMemFraction = 0.65;
    const size_t afford = std::max(capacity, (size_t)((double)(free_b / std::max(1u, share) + capacity * per_path) * kPassMemFraction) / per_path);
    const size_t paths = std::min(afford, kPassMaxPaths / std::max(1u, share));
    uint32_t S = (uint32_t)std::min<size_t>(spp, std::max<size_t>(1, paths / std::max(1u, n_pix_slots)));
    const uint32_t n_pass = (spp + S - 1) / S;
    return (spp + n_pass - 1) / n_pass;
}

int main() {
    const uint32_t n_pix = 256;
    struct Named { const char *name; PassBudget b; uint32_t K; };
    const std::vector<Named> budgets = {
        {"path", {0, 0.65, (size_t)1 << 29}, 0}, {"aov", {32, 0.5, (size_t)1 << 29}, 0},
        {"ao K=1", {4 + 1 * 40, 0.5, ((size_t)1 << 31) / 1}, 1}, {"ao K=64", {4 + 64 * 40, 0.5, ((size_t)1 << 31) / 64}, 64},
        {"cap of 3 samples", {0, 0.65, 3 * 256}, 0}, {"cap of 5 samples, ao K=64", {4 + 64 * 40, 0.5, 5 * 256 + 17}, 64}};
    size_t n_cases = 0;
    for (const Named &nb : budgets) for (size_t workspace : {(size_t)256 + 4 * 13, (size_t)256 + 4 * 31}) for (uint32_t share : {1u, 2u}) for (uint32_t held_samples : {0u, 2u, 5u})
    for (uint32_t n = 1; n <= 7; ++n) {
        const PassBudget &b = nb.b;
        const size_t per_path = workspace + b.extra_bytes_per_path, held = (size_t)held_samples * n_pix * workspace;
        // free memory: nothing, and around every boundary at which one more sample per pass becomes affordable, and plenty
        std::vector<size_t> frees = {0, 1, (size_t)1 << 40};
        for (uint32_t s = 1; s <= 8; ++s) {
            const double need = (double)s * n_pix * per_path / b.mem_fraction - (double)held;
            if (need <= 0.0) continue;
            for (long d : {-(long)per_path, -1L, 0L, 1L, (long)per_path, 2L * (long)per_path}) { const double f = need * share + (double)d; if (f >= 0.0) frees.push_back((size_t)f); }
        }
        for (size_t free_b : frees) {
            ++n_cases;
            const uint32_t S = pass_size_for(free_b, held, per_path, b, n_pix, n, share);
            const double limit = (double)(free_b / share + held) * b.mem_fraction;
            const size_t cap = b.max_paths / share;
            auto within = [&](uint32_t s) { return ((double)s * n_pix * per_path <= limit || (size_t)s * n_pix * per_path <= held) && (size_t)s * n_pix <= cap; };
            CHECK(S >= 1 && S <= n, "%s: S = %u of n = %u", nb.name, S, n);
            if (S == 0) continue;
            const uint32_t n_pass = (n + S - 1) / S;
            CHECK((n + n_pass - 1) / n_pass == S, "%s: passes of S = %u over n = %u are not equal", nb.name, S, n);
            CHECK(S == 1 || within(S), "%s: S = %u needs %.0f bytes, the budget is %.0f (free %zu, held %zu, share %u), cap %zu paths", nb.name, S, (double)S * n_pix * per_path, limit, free_b, held, share, cap);
            // the largest size within the budget, made equal: no pass count below n_pass fits
            if (n_pass > 1) { const uint32_t larger = (n + n_pass - 2) / (n_pass - 1); CHECK(!within(larger), "%s: %u passes of %u would fit, chose %u of %u (n = %u, free %zu, held %zu)", nb.name, n_pass - 1, larger, n_pass, S, n, free_b, held); }
            if (nb.K) CHECK((size_t)n_pix * S * nb.K <= ((size_t)1 << 31), "%s: %u x %u x %u rays", nb.name, n_pix, S, nb.K);
            if (b.extra_bytes_per_path == 0 && b.max_paths == (size_t)1 << 29)
                CHECK(S == former_path_rule(free_b, held / workspace, workspace, n_pix, n, share), "path: S = %u, the former rule chose %u", S, former_path_rule(free_b, held / workspace, workspace, n_pix, n, share));
        }
    }
    // exact figures: 308 bytes per path, 256 slots: 0.65 of the memory holds three samples' paths and not four -> 7 samples in passes of 3, 2, 2 become 3 equal passes of 3
    {
        const PassBudget path{0, 0.65, (size_t)1 << 29};
        const size_t three = (size_t)(3.5 * 256 * 308 / 0.65);
        CHECK(pass_size_for(three, 0, 308, path, 256, 7, 1) == 3, "got %u", pass_size_for(three, 0, 308, path, 256, 7, 1));
        CHECK(pass_size_for(three, 0, 308, path, 256, 6, 1) == 3, "got %u", pass_size_for(three, 0, 308, path, 256, 6, 1));
        CHECK(pass_size_for(three, 0, 308, path, 256, 4, 1) == 2, "got %u", pass_size_for(three, 0, 308, path, 256, 4, 1));   // 3 + 1 -> 2 + 2
        CHECK(pass_size_for(three, 0, 308, path, 256, 7, 2) == 1, "got %u", pass_size_for(three, 0, 308, path, 256, 7, 2));   // half the memory: one sample
        CHECK(pass_size_for(0, 5 * 256 * 308, 308, path, 256, 7, 1) == 4, "got %u", pass_size_for(0, 5 * 256 * 308, 308, path, 256, 7, 1));   // the workspace that exists: 5 -> 7 in 2 passes of 4
        // the queues that exist, not a bound on them: at 13 queues a path costs 308 + 32 bytes with its feature record, not 256 + 4 x 28 + 32
        const PassBudget aov{32, 0.5, (size_t)1 << 29};
        const size_t mem = (size_t)(7.0 * 256 * 340 / 0.5) + 1;
        CHECK(pass_size_for(mem, 0, 340, aov, 256, 7, 1) == 7, "got %u", pass_size_for(mem, 0, 340, aov, 256, 7, 1));
        CHECK(pass_size_for(mem, 0, 256 + 4 * 28 + 32, aov, 256, 7, 1) == 4, "got %u", pass_size_for(mem, 0, 256 + 4 * 28 + 32, aov, 256, 7, 1));   // (what the stale constant made of the same memory: 5 affordable -> 4 + 3 -> 4)
    }
    // nothing to divide by
    {
        const PassBudget path{0, 0.65, (size_t)1 << 29};
        CHECK(pass_size_for(0, 0, 308, path, 0, 7, 1) == 1, "no pixel slots, no memory");
        CHECK(pass_size_for((size_t)1 << 30, 0, 308, path, 0, 7, 1) == 7, "no pixel slots");
        CHECK(pass_size_for(0, 0, 308, path, 256, 7, 1) == 1, "no memory");
        CHECK(pass_size_for(0, 0, 0, path, 256, 7, 0) == 1, "no bytes per path, no share");
        CHECK(pass_size_for((size_t)1 << 30, 0, 308, path, 256, 0, 1) == 1, "no samples");
        CHECK(pass_size_for((size_t)1 << 30, 0, 308, PassBudget{0, 0.65, 0}, 256, 7, 1) == 1, "no paths allowed");
    }
    std::printf("check_pass_budget: %zu cases, %d failed\n", n_cases, g_failed);
    return g_failed ? 1 : 0;
}
