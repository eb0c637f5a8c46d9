// Optional per-launch timing of the convolution launches (bench.py's roofline leg): the library's only mutable global
// state, touched by the host thread only.  Off by default.  Interface and category numbering: conv_igemm_host.h.
// Entry points: objgan_prof_enable, objgan_prof_collect, objgan_prof_dump.  No kernels.
#include "conv_igemm_host.h"

#define OG_PROF_MAX 65536
struct ProfRec { hipEvent_t a, b; int cat; double flops; int meta[10]; };
static int g_prof_on = 0;
static ProfRec* g_prof = nullptr;
static int g_prof_n = 0;
static int g_prof_made = 0;

ProfRec* prof_begin(int cat, double flops, hipStream_t s) {
    if (!g_prof_on || g_prof_n >= OG_PROF_MAX) return nullptr;
    if (!g_prof) g_prof = (ProfRec*)calloc(OG_PROF_MAX, sizeof(ProfRec));
    ProfRec* r = &g_prof[g_prof_n];
    if (g_prof_n >= g_prof_made) {
        if (hipEventCreate(&r->a) != hipSuccess || hipEventCreate(&r->b) != hipSuccess) return nullptr;
        g_prof_made = g_prof_n + 1;
    }
    g_prof_n++;
    r->cat = cat; r->flops = flops;
    for (int i = 0; i < 10; ++i) r->meta[i] = 0;
    (void)hipEventRecord(r->a, s);
    return r;
}
void prof_meta(ProfRec* r, int kind, int tm, int M, int C, int T, int N, int ph, int pw, int stride, int splits) {
    if (!r) return;
    const int v[10] = {kind, tm, M, C, T, N, ph, pw, stride, splits};
    for (int i = 0; i < 10; ++i) r->meta[i] = v[i];
}
void prof_end(ProfRec* r, hipStream_t s) { if (r) (void)hipEventRecord(r->b, s); }

extern "C" {

int objgan_prof_enable(int on) {
    OG_ENTRY();
    g_prof_on = on ? 1 : 0;
    if (on) {
        g_prof_n = 0;
        // create the whole event pool up front: hipEventCreate inside the measured region would
        // cost the host tens of milliseconds per step
        if (!g_prof) g_prof = (ProfRec*)calloc(OG_PROF_MAX, sizeof(ProfRec));
        while (g_prof && g_prof_made < OG_PROF_MAX) {
            ProfRec* r = &g_prof[g_prof_made];
            if (hipEventCreate(&r->a) != hipSuccess || hipEventCreate(&r->b) != hipSuccess) break;
            g_prof_made++;
        }
    }
    return OG_OK;
}

// Sums the recorded launches per category (the caller must have synchronised the device).
// ms, flops, count: arrays of OG_PROF_CATS = 192.  Categories = kernel instances (og_prof_cat, conv_igemm_host.h).
int objgan_prof_collect(double* ms, double* flops, long* count) {
    OG_ENTRY();
    for (int i = 0; i < OG_PROF_CATS; ++i) { ms[i] = 0; flops[i] = 0; count[i] = 0; }
    for (int i = 0; i < g_prof_n; ++i) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, g_prof[i].a, g_prof[i].b) != hipSuccess) continue;
        ms[g_prof[i].cat] += t; flops[g_prof[i].cat] += g_prof[i].flops; count[g_prof[i].cat] += 1;
    }
    g_prof_n = 0;
    return OG_OK;
}

// Per-launch records of the last profiling window (device must be idle): ms[i], flops[i], meta[10*i..]
// (see ProfRec::meta), at most max_records; *n_out = number written.  Does not reset the window.
int objgan_prof_dump(float* ms, double* flops, int* meta, int max_records, int* n_out) {
    OG_ENTRY();
    int n = 0;
    for (int i = 0; i < g_prof_n && n < max_records; ++i) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, g_prof[i].a, g_prof[i].b) != hipSuccess) continue;
        ms[n] = t; flops[n] = g_prof[i].flops;
        for (int j = 0; j < 10; ++j) meta[10 * n + j] = g_prof[i].meta[j];
        ++n;
    }
    if (n_out) *n_out = n;
    return OG_OK;
}

}  // extern "C"
