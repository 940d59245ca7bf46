// TEST INFRASTRUCTURE -- CPU shim of the depth encoder's backward pass (isaacgymloco_amd/csrc/ls_depth_encoder_bwd.h): the validation, both plans,
// the split of the samples over the workgroups (ls_deb_first / ls_deb_count), the index arithmetic (ls_de_slot, ls_de_tap, ls_de_base and their
// tables, ls_deb_dz, ls_deb_delu, ls_deb_da1, the layout of a partial sum) and the order in which the partial sums are added are the kernels' own;
// the workgroups run one after the other, each on an "LDS" of the planned size, and the sums the kernels form on MFMA tiles are plain fp32
// loops here.  The entry points carry the signatures of include/lsim.h (the stream is ignored).
#define LS_EMU 1
#include "../../isaacgymloco_amd/csrc/ls_depth_encoder_bwd.h"
#include <vector>

static void emu_deb_conv(const float* in, float* out, const int* tap, const int* base, const float* w, const float* b, int K, int cout, int P) {
    for (int c = 0; c < cout; ++c)
        for (int pos = 0; pos < P; ++pos) {
            float acc = 0.0f;
            for (int kk = 0; kk < K; ++kk) acc += w[(size_t)c * K + kk] * in[tap[kk] + base[pos]];
            out[c * P + pos] = ls_de_elu(acc + b[c]);
        }
}
// ls_deb_wgrad: one sample's weight and bias gradient of a layer added to the partial sum (stored when `first`)
static void emu_deb_wgrad(const float* d, const float* in, const int* tap, const int* base, int K, int cout, int P, float* pw, float* pb, bool first) {
    for (int c = 0; c < cout; ++c) {
        for (int kk = 0; kk < K; ++kk) {
            float acc = 0.0f;
            for (int pos = 0; pos < P; ++pos) acc += d[c * P + pos] * in[tap[kk] + base[pos]];
            float* dst = pw + (size_t)c * K + kk;
            *dst = first ? acc : *dst + acc;
        }
        float v = 0.0f;
        for (int pos = 0; pos < P; ++pos) v += d[c * P + pos];
        pb[c] = first ? v : pb[c] + v;
    }
}

// the sample split, for the tests to read (no lsim_ counterpart)
extern "C" int emu_deb_first(int k, int batch, int G) { return ls_deb_first(k, batch, G); }
extern "C" int emu_deb_count(int k, int batch, int G) { return ls_deb_count(k, batch, G); }

extern "C" int emu_depth_encode_backward_sizes(const lsim_depth_encoder_bwd_t* db, size_t* lds_bytes, size_t* workspace_bytes) {
    return ls_deb_sizes(db, lds_bytes, workspace_bytes);
}

extern "C" int emu_depth_encode_backward(const lsim_depth_encoder_bwd_t* dbp, void* /*stream*/) {
    lsim_depth_encoder_t de;
    LsDePlan p;
    LsDebPlan q;
    const int rv = ls_deb_validate(dbp, de, p, q);
    if (rv != LSIM_OK) return rv;
    const lsim_depth_encoder_bwd_t& db = *dbp;
    float* ws = (float*)db.workspace;
    const int R = de.height * de.width, L = de.latent_dim, K3 = p.K3;
    std::vector<float> lds((size_t)q.words);
    // launch 1: workgroup k over its samples
    for (int k = 0; k < q.G; ++k) {
        for (size_t w = 0; w < lds.size(); ++w) lds[w] = -1.0e30f;           // LDS is not initialised
        float* X = lds.data();
        float* A1 = X + q.oA1;
        float* A2 = X + q.oA2;
        float* DZ = X + q.oDZ;
        int* T1 = (int*)(X + q.oT1);
        int* T2 = (int*)(X + q.oT2);
        int* B1 = (int*)(X + q.oB1);
        int* B2 = (int*)(X + q.oB2);
        for (int kk = 0; kk < p.K1; ++kk) T1[kk] = ls_de_tap(kk, de.k1, de.height, de.width);
        for (int kk = 0; kk < p.K2; ++kk) T2[kk] = ls_de_tap(kk, de.k2, p.h1, p.w1);
        for (int pos = 0; pos < q.P1; ++pos) B1[pos] = ls_de_base(pos, p.w1, de.s1, de.width);
        for (int pos = 0; pos < q.P2; ++pos) B2[pos] = ls_de_base(pos, p.w2, de.s2, p.w1);
        float* part = ws + q.wsPart + (size_t)k * (size_t)q.NP;
        const int b0 = ls_deb_first(k, db.batch, q.G), nb = ls_deb_count(k, db.batch, q.G);
        for (int s = 0; s < nb; ++s) {
            const int b = b0 + s;
            const bool first = s == 0;
            for (int f = 0; f < de.frames; ++f)
                for (int r = 0; r < R; ++r) X[f * R + r] = de.hist[ls_de_slot(de, b, f) + (size_t)r];
            for (int o = 0; o < L; ++o) {
                const float v = ls_deb_dz(db.g[(size_t)b * db.g_stride + o], db.latent[(size_t)b * db.latent_stride + o], db.final_act);
                DZ[o] = v;
                ws[(size_t)q.wsDZ + (size_t)b * L + o] = v;
            }
            emu_deb_conv(X, A1, T1, B1, de.w1, de.b1, p.K1, de.c1, q.P1);
            emu_deb_conv(A1, A2, T2, B2, de.w2, de.b2, p.K2, de.c2, q.P2);
            for (int j = 0; j < K3; ++j) {
                const float a = A2[j];
                ws[(size_t)b * K3 + j] = a;
                float acc = 0.0f;
                for (int o = 0; o < L; ++o) acc += de.w3[(size_t)o * K3 + j] * DZ[o];
                A2[j] = acc * ls_deb_delu(a);
            }
            emu_deb_wgrad(A2, A1, T2, B2, p.K2, de.c2, q.P2, part + ls_deb_part_gw2(de.c1, p.K1), part + ls_deb_part_gb2(de.c1, p.K1, de.c2, p.K2), first);
            for (int e = 0; e < de.c1 * q.P1; ++e) {
                const int d = e / q.P1, pos = e - d * q.P1, Y = pos / p.w1, Xc = pos - Y * p.w1;
                const float da = ls_deb_da1(A2, de.w2, d, Y, Xc, de.c1, de.c2, de.k2, de.s2, p.h2, p.w2);
                A1[e] = da * ls_deb_delu(A1[e]);
            }
            emu_deb_wgrad(A1, X, T1, B1, p.K1, de.c1, q.P1, part, part + ls_deb_part_gb1(de.c1, p.K1), first);
        }
    }
    // launch 2: gw3 | gb3 over the workspace rows, b ascending
    for (int o = 0; o < L; ++o) {
        for (int j = 0; j < K3; ++j) {
            float acc = 0.0f;
            for (int b = 0; b < db.batch; ++b) acc += ws[(size_t)q.wsDZ + (size_t)b * L + o] * ws[(size_t)b * K3 + j];
            db.gw3[(size_t)o * K3 + j] = acc;
        }
        float acc = 0.0f;
        for (int b = 0; b < db.batch; ++b) acc += ws[(size_t)q.wsDZ + (size_t)b * L + o];
        db.gb3[o] = acc;
    }
    // launch 3: the partial sums in the order of the workgroups
    const int ob1 = ls_deb_part_gb1(de.c1, p.K1), ow2 = ls_deb_part_gw2(de.c1, p.K1), ob2 = ls_deb_part_gb2(de.c1, p.K1, de.c2, p.K2);
    for (int idx = 0; idx < q.NP; ++idx) {
        float v = ws[q.wsPart + idx];
        for (int k = 1; k < q.G; ++k) v += ws[q.wsPart + (size_t)k * (size_t)q.NP + idx];
        if (idx < ob1) db.gw1[idx] = v;
        else if (idx < ow2) db.gb1[idx - ob1] = v;
        else if (idx < ob2) db.gw2[idx - ow2] = v;
        else db.gb2[idx - ob2] = v;
    }
    return LSIM_OK;
}
