// check_cli_plan.cpp -- a stand-alone check of the host-only part of mi355pbrt's command line (frontend/cli_plan.h) on the CPU: no HIP, no device, plain g++.
//
// Without arguments it exits 0 when all of this holds:
//   * groups(): for first <= last in 0..9, group sizes 1, 2, 3, 7 and last - first, samples_done in 0..last - first, with and without --denoise (with: two samples at
//     least, as make_plan grants) -- the groups are contiguous, cover exactly [first + samples_done, last), and each has 1 <= n <= group size;
//   * under --denoise no group holds both mid - 1 and mid, `half` is 0 before mid and 1 from it on, and both halves get a group when samples_done is 0; without it
//     `half` is always 0, and a group size of last - first gives one group -- the plain run's single pt_render_samples call;
//   * make_plan(): --spp replaces the job's spp, [first, last) is --samples or the whole job, mid == first + (last - first) / 2, the film's size is the cropped window's,
//     an empty film is status 1 "empty film"; the lenient numbers (--spp 8x is 8) stay.
// `check_cli_plan verdict SPP IS_AO ARGS...` prints what mi355pbrt decides about the command line `mi355pbrt ARGS...` before it touches the device: a line
// "parse <status>" or, when parse_options accepts it and SPP > 0, "plan <status>" from make_plan on a 16x16 job of SPP samples per pixel (IS_AO: of the
// ambient-occlusion integrator), then the message. tests/test_cli_refusals.py runs its table of refused command lines through it.
#include "cli_plan.h"
#include <cstdio>
#include <initializer_list>

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_failed <= 20) { std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static PtRenderParams job(uint32_t spp, int x0, int y0, int x1, int y1) {
    PtRenderParams rp{};
    rp.spp = spp;
    rp.cropped_pixel_bounds[0] = x0; rp.cropped_pixel_bounds[1] = y0; rp.cropped_pixel_bounds[2] = x1; rp.cropped_pixel_bounds[3] = y1;
    return rp;
}

static int verdict(int argc, char **argv) {
    const uint32_t spp = (uint32_t)std::atoi(argv[2]); const bool is_ao = std::atoi(argv[3]) != 0;
    Options o; Plan p; std::string why;
    argv[3] = argv[0];   // parse_options reads from argv[1] on
    int st = parse_options(argc - 3, argv + 3, o, why);
    const char *stage = "parse";
    if (st == 0 && spp > 0) { stage = "plan"; st = make_plan(o, job(spp, 0, 0, 16, 16), is_ao, p, why); }
    std::printf("%s %d\n%s\n", stage, st, why.c_str());
    return 0;
}

static size_t check_groups() {
    size_t n_cases = 0;
    for (uint32_t first = 0; first <= 9; ++first) for (uint32_t last = first; last <= 9; ++last) for (int dn = 0; dn <= (last - first >= 2 ? 1 : 0); ++dn) {
        Plan p{}; p.first = first; p.last = last; p.mid = first + (last - first) / 2; p.denoise = dn != 0;
        for (uint32_t size : {1u, 2u, 3u, 7u, last - first}) for (uint32_t done = 0; size > 0 && done <= last - first; ++done, ++n_cases) {
            const std::vector<Group> g = groups(p, size, done);
            uint32_t s = first + done; bool in_a = false, in_b = false;
            for (const Group &k : g) {
                CHECK(k.first == s, "[%u, %u) dn %d size %u done %u: a group begins at %u, not %u", first, last, dn, size, done, k.first, s);
                CHECK(k.n >= 1 && k.n <= size, "[%u, %u) dn %d size %u done %u: a group of %u", first, last, dn, size, done, k.n);
                CHECK(k.half == (dn && k.first >= p.mid ? 1 : 0), "[%u, %u) dn %d size %u done %u: group at %u has half %d", first, last, dn, size, done, k.first, k.half);
                if (dn) CHECK(!(k.first < p.mid && k.first + k.n > p.mid), "[%u, %u) size %u done %u: group [%u, %u) crosses mid %u", first, last, size, done, k.first, k.first + k.n, p.mid);
                (k.half ? in_b : in_a) = true;
                s += k.n;
            }
            CHECK(s == last, "[%u, %u) dn %d size %u done %u: the groups end at %u", first, last, dn, size, done, s);
            if (dn && done == 0) CHECK(in_a && in_b, "[%u, %u) size %u: a half without a group", first, last, size);
            if (!dn && done == 0 && size == last - first) CHECK(g.size() == 1 && g[0].first == first && g[0].n == size, "[%u, %u): %zu groups for the whole run", first, last, g.size());
        }
        CHECK(groups(p, 3, last - first).empty(), "[%u, %u) dn %d: groups after the last sample", first, last, dn);
    }
    return n_cases;
}

static size_t check_make_plan() {
    size_t n_cases = 0;
    for (uint32_t job_spp : {1u, 2u, 5u, 8u, 9u}) for (int spp_flag : {0, 1, 4, 7}) for (const char *samples : {"", "0:1", "1:4", "2:7", "0:9"}) for (int dn = 0; dn <= 1; ++dn, ++n_cases) {
        Options o; Plan p; std::string why;
        const char *argv[10] = {"mi355pbrt", "scene.pbrt"}; int argc = 2;
        const std::string spp_text = std::to_string(spp_flag) + "x";   // (atoi: the digits count)
        if (spp_flag) { argv[argc++] = "--spp"; argv[argc++] = spp_text.c_str(); }
        if (*samples) { argv[argc++] = "--samples"; argv[argc++] = samples; }
        if (dn) { argv[argc++] = "--denoise"; argv[argc++] = "d.pfm"; }
        CHECK(parse_options(argc, (char **)argv, o, why) == 0 && why.empty(), "spp %d samples \"%s\" dn %d: refused: %s", spp_flag, samples, dn, why.c_str());
        const uint32_t spp = spp_flag ? (uint32_t)spp_flag : job_spp;
        const uint32_t first = *samples ? (uint32_t)(samples[0] - '0') : 0, last = *samples ? (uint32_t)(samples[2] - '0') : spp;
        const int st = make_plan(o, job(job_spp, 3, 5, 43, 29), false, p, why);
        const int want = last > spp || (dn && last - first < 2) ? 2 : 0;
        CHECK(st == want, "job %u spp %d samples \"%s\" dn %d: status %d (%s), expected %d", job_spp, spp_flag, samples, dn, st, why.c_str(), want);
        if (st == 0 && want == 0) {
            CHECK(p.rp.spp == spp && p.first == first && p.last == last && p.mid == first + (last - first) / 2 && p.denoise == (dn != 0) && p.width == 40 && p.height == 24,
                  "job %u spp %d samples \"%s\" dn %d: spp %u [%u, %u) mid %u, %d x %d", job_spp, spp_flag, samples, dn, p.rp.spp, p.first, p.last, p.mid, p.width, p.height);
            if (dn) CHECK(p.first < p.mid && p.mid < p.last, "[%u, %u): mid %u leaves a half empty", p.first, p.last, p.mid);
        }
    }
    for (int x1 : {3, 2}) {   // no column, a negative width
        Options o; Plan p; std::string why; ++n_cases;
        CHECK(make_plan(o, job(4, 3, 0, x1, 8), false, p, why) == 1 && why == "empty film", "a film of %d columns: %s", x1 - 3, why.c_str());
    }
    return n_cases;
}

int main(int argc, char **argv) {
    if (argc >= 4 && std::string(argv[1]) == "verdict") return verdict(argc, argv);
    const size_t n_groups = check_groups(), n_plans = check_make_plan();
    std::printf("check_cli_plan: %zu group lists, %zu plans, %d failed\n", n_groups, n_plans, g_failed);
    return g_failed ? 1 : 0;
}
