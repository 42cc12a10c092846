// tools/study/ray_order_model.cpp -- CPU model of "which rays sit next to each other in a wave": the production walk (the reference's binary SAH tree, two levels per record,
// reference order, one packet per primitive) logs the sequence of records and packets every ray fetches; waves of 64 consecutive queue entries then run in lock step (step s =
// every lane's s-th fetch) and the model counts the DISTINCT lines a wave asks for per step and over its whole life. Counts only: plain float arithmetic, no parity claims.
// Driven by tools/study/ray_order_model.py; the walk is the one of wide_study.cpp (walker A) with a log.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

struct Node { float bmin[3], bmax[3]; uint32_t offset; uint16_t n_prims; uint8_t axis, pad; };   // PtBVHNode (include/mi355pt.h)
struct Ray { float o[3], d[3], tmax; uint32_t any; };

static const Node *N; static const uint32_t *ORD; static const float *P; static const uint32_t *IDX;
static std::vector<uint32_t> LOG;        // every ray's fetches, ray after ray: a record = its node index, a packet = 0x80000000 | its slot in the ordered primitive list
static std::vector<uint64_t> LOG_AT;     // ray r's fetches are LOG[LOG_AT[r] .. LOG_AT[r + 1])

static inline bool slab(const float *bmin, const float *bmax, const Ray &r, const float *inv, float tmax, float &tmin_out) {
    float tmin = 0.0f, tmx = tmax;
    for (int a = 0; a < 3; ++a) {
        float t0 = (bmin[a] - r.o[a]) * inv[a], t1 = (bmax[a] - r.o[a]) * inv[a];
        if (inv[a] < 0.0f) std::swap(t0, t1);
        t1 *= 1.0000004f;
        if (t0 > tmin) tmin = t0;
        if (t1 < tmx) tmx = t1;
        if (tmin > tmx) return false;
    }
    tmin_out = tmin; return true;
}
static inline bool tri_hit(uint32_t prim, const Ray &r, float tmax, float &t) {   // Moeller-Trumbore (counts only)
    const float *p0 = P + 3 * IDX[3 * prim], *p1 = P + 3 * IDX[3 * prim + 1], *p2 = P + 3 * IDX[3 * prim + 2];
    float e1[3], e2[3], pv[3], tv[3], qv[3];
    for (int k = 0; k < 3; ++k) { e1[k] = p1[k] - p0[k]; e2[k] = p2[k] - p0[k]; }
    pv[0] = r.d[1] * e2[2] - r.d[2] * e2[1]; pv[1] = r.d[2] * e2[0] - r.d[0] * e2[2]; pv[2] = r.d[0] * e2[1] - r.d[1] * e2[0];
    const float det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
    if (det == 0.0f) return false;
    const float inv = 1.0f / det;
    for (int k = 0; k < 3; ++k) tv[k] = r.o[k] - p0[k];
    const float u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) * inv;
    if (u < 0.0f || u > 1.0f) return false;
    qv[0] = tv[1] * e1[2] - tv[2] * e1[1]; qv[1] = tv[2] * e1[0] - tv[0] * e1[2]; qv[2] = tv[0] * e1[1] - tv[1] * e1[0];
    const float v = (r.d[0] * qv[0] + r.d[1] * qv[1] + r.d[2] * qv[2]) * inv;
    if (v < 0.0f || u + v > 1.0f) return false;
    t = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) * inv;
    return t > 1e-6f * std::fabs(t) && t < tmax;
}

// The production walk with a log; returns the closest hit's t (the ray's tmax on a miss).
static float walk_logged(const Ray &r, std::vector<uint32_t> *log) {
    float inv[3] = {1.0f / r.d[0], 1.0f / r.d[1], 1.0f / r.d[2]};
    const bool neg[3] = {inv[0] < 0, inv[1] < 0, inv[2] < 0};
    float tmax = r.tmax;
    struct E { uint32_t node; float tmin; };
    E stack[128]; int sp = 0;
    uint32_t cur = 0; bool have = true;
    for (;;) {
        if (have) {
            const Node &n = N[cur];
            if (n.n_prims) {
                for (uint32_t i = 0; i < n.n_prims; ++i) {
                    if (log) log->push_back(0x80000000u | (n.offset + i));
                    float t; if (tri_hit(ORD[n.offset + i], r, tmax, t)) { if (r.any) return t; tmax = t; }
                }
                have = false;
            } else {
                if (log) log->push_back(cur);
                uint32_t slots[4]; int ns = 0;
                const uint32_t L = cur + 1, R = n.offset;
                const uint32_t order[2] = {neg[n.axis] ? R : L, neg[n.axis] ? L : R};
                for (uint32_t x : order) {
                    if (N[x].n_prims) slots[ns++] = x;
                    else { const uint32_t a = x + 1, b = N[x].offset; if (neg[N[x].axis]) { slots[ns++] = b; slots[ns++] = a; } else { slots[ns++] = a; slots[ns++] = b; } }
                }
                float T[4]; bool ok[4];
                for (int k = 0; k < ns; ++k) ok[k] = slab(N[slots[k]].bmin, N[slots[k]].bmax, r, inv, tmax, T[k]);
                int first = -1;
                for (int k = 0; k < ns; ++k) if (ok[k]) { first = k; break; }
                if (first < 0) have = false;
                else { for (int k = ns - 1; k > first; --k) if (ok[k]) stack[sp++] = {slots[k], T[k]}; cur = slots[first]; }
            }
        }
        if (!have) {
            bool found = false;
            while (sp > 0) { const E e = stack[--sp]; if (e.tmin < tmax) { cur = e.node; found = true; break; } }
            if (!found) break;
            have = true;
        }
    }
    return tmax;
}

static size_t distinct(std::vector<uint32_t> &v) { std::sort(v.begin(), v.end()); return (size_t)(std::unique(v.begin(), v.end()) - v.begin()); }

extern "C" {
void model_set(const Node *nodes, const uint32_t *ordered, const float *p, const uint32_t *idx) { N = nodes; ORD = ordered; P = p; IDX = idx; }
// closest hit of n rays: t (inf = miss)
void model_closest(const Ray *rays, uint32_t n, float *t) { for (uint32_t i = 0; i < n; ++i) t[i] = walk_logged(rays[i], nullptr); }
// log the fetch sequence of n rays (replaces the previous log); returns the number of fetches
uint64_t model_log(const Ray *rays, uint32_t n) {
    LOG.clear(); LOG_AT.assign(1, 0);
    for (uint32_t i = 0; i < n; ++i) { walk_logged(rays[i], &LOG); LOG_AT.push_back(LOG.size()); }
    return LOG.size();
}
// The logged rays in the queue order `order` (n entries), waves of `wave` consecutive entries in lock step.
// out: [0] lane fetches, [1] sum over wave-steps of the distinct lines, [2] sum over waves of the distinct lines.
void model_waves(const uint32_t *order, uint32_t n, uint32_t wave, double *out) {
    out[0] = out[1] = out[2] = 0.0;
    std::vector<uint32_t> step, whole;
    for (uint32_t w0 = 0; w0 < n; w0 += wave) {
        const uint32_t w1 = std::min(n, w0 + wave);
        uint64_t longest = 0; whole.clear();
        for (uint32_t e = w0; e < w1; ++e) { const uint32_t r = order[e]; longest = std::max(longest, LOG_AT[r + 1] - LOG_AT[r]); whole.insert(whole.end(), LOG.begin() + LOG_AT[r], LOG.begin() + LOG_AT[r + 1]); }
        out[0] += (double)whole.size(); out[2] += (double)distinct(whole);
        for (uint64_t s = 0; s < longest; ++s) {
            step.clear();
            for (uint32_t e = w0; e < w1; ++e) { const uint32_t r = order[e]; if (LOG_AT[r] + s < LOG_AT[r + 1]) step.push_back(LOG[LOG_AT[r] + s]); }
            out[1] += (double)distinct(step);
        }
    }
}
// The logged rays in groups of `group` consecutive rays (one origin's rays): sum of the groups' distinct fetches / sum of their fetches.
double model_groups(uint32_t n, uint32_t group) {
    double d = 0.0; std::vector<uint32_t> g;
    for (uint32_t r0 = 0; r0 + group <= n; r0 += group) { g.assign(LOG.begin() + LOG_AT[r0], LOG.begin() + LOG_AT[r0 + group]); d += (double)distinct(g); }
    return LOG.empty() ? 0.0 : d / (double)LOG_AT[n - n % group];
}
}
