// hostcheck_mcmc.hip -- TEST SHIM: runs the product's per-Gaussian 3DGS-MCMC arithmetic (reduced-3dgs_amd/csrc/mcmc_math.h, the
// __host__ __device__ functions csrc/mcmc.hip executes per lane) on the CPU, so tests/test_mcmc_cpu.py can compare it with the
// numpy restatement WITHOUT a GPU.  Not part of the product; nothing in reduced-3dgs_amd/ links it.
// Built twice: as a shared library the test loads with ctypes, and -- with -DHOSTCHECK_MCMC_MAIN -- as a stand-alone program
// that sweeps the same functions over edge inputs, which the test also compiles with -fsanitize=address,undefined on the host
// side and runs on its own (nothing that carries a sanitizer is loaded into Python).
#include "../../reduced-3dgs_amd/csrc/mcmc_math.h"

#include <cstdio>
#include <vector>

static const r3::McmcBinom kBinom = r3::make_mcmc_binom();

extern "C" {

double hc_mcmc_binom(int n, int k) { return kBinom.c[n][k]; }

void hc_mcmc_gate(int n, const float* o, float* out)
{
    for (int i = 0; i < n; i++) out[i] = r3::mcmc_gate(o[i]);
}

// noise_kernel's per-lane body: xyz [n,3] in place
void hc_mcmc_noise(int n, float* xyz, const float* opacity, const float* scaling, const float* rotation, const float* noise,
                   float scale)
{
    for (int i = 0; i < n; i++) {
        float d[3];
        r3::mcmc_noise_delta(rotation + 4 * i, scaling + 3 * i, opacity[i], noise + 3 * i, scale, d);
        for (int k = 0; k < 3; k++) xyz[3 * i + k] = r3::mcmc_displace(xyz[3 * i + k], d[k]);
    }
}

// weights_kernel's and cdf_kernel's per-lane body and the compaction, sequentially: -> the number of rows of positive weight
int hc_mcmc_weights(int n, const float* opacity, float min_opacity, int relocate, float* w, unsigned char* dead, double* cdf,
                    int* idx)
{
    double run = 0.0;
    int pos = 0;
    for (int i = 0; i < n; i++) {
        bool d;
        w[i] = r3::mcmc_weight(opacity[i], min_opacity, relocate, d);
        dead[i] = d;
        run += (double)w[i];
        if (w[i] > 0.f) {
            cdf[pos] = run;
            idx[pos++] = i;
        }
    }
    return pos;
}

// draw_kernel's per-lane body over a compacted cdf of `pos` rows
void hc_mcmc_draw(int pos, const double* cdf, const int* idx, double total, int n, const float* u, int* sampled)
{
    for (int k = 0; k < n; k++) sampled[k] = idx[r3::mcmc_search(cdf, pos, r3::mcmc_target(u[k], total))];
}

int hc_mcmc_ratio_clamp(int r) { return r3::mcmc_ratio_clamp(r); }

void hc_mcmc_relocate_f64(double o, int N, double* o_new, double* D) { r3::mcmc_relocate_f64(o, N, kBinom, *o_new, *D); }

// values_kernel's per-lane body
void hc_mcmc_relocate(int n, const float* opacity, const float* scaling, const int* ratio, float min_opacity, float* new_opacity,
                      float* new_scaling)
{
    for (int i = 0; i < n; i++) r3::mcmc_relocate(opacity[i], scaling + 3 * i, ratio[i], min_opacity, kBinom, new_opacity[i], new_scaling + 3 * i);
}

}  // extern "C"

#ifdef HOSTCHECK_MCMC_MAIN
// Every function over its edge inputs; prints a checksum so that nothing is optimised away.  Exit status 1 on a broken
// invariant (a draw of a row of weight zero, a ratio above the clamp, a non-finite relocation).
int main()
{
    int bad = 0;
    double sum = 0.0;
    const int n = 1000;
    std::vector<float> op(n), sc(3 * n), rot(4 * n), nz(3 * n), xyz(3 * n), w(n), no(n), ns(3 * n);
    std::vector<unsigned char> dead(n);
    std::vector<double> cdf(n);
    std::vector<int> idx(n), ratio(n), sampled(n);
    for (int i = 0; i < n; i++) {
        op[i] = i % 7 == 0 ? -20.f : (i % 11 == 0 ? 20.f : -6.f + 0.011f * i);
        ratio[i] = 1 + i % 51;
        for (int k = 0; k < 3; k++) {
            sc[3 * i + k] = -7.f + 0.007f * i + k;
            nz[3 * i + k] = i % 5 ? 0.3f * (k - 1) + 0.001f * i : 0.f;
            xyz[3 * i + k] = i % 2 ? -0.f : 1.f + k;
        }
        for (int k = 0; k < 4; k++) rot[4 * i + k] = i == 3 ? 0.f : (0.1f + k) * (i % 3 == 0 ? 1e-6f : 7.f) * (k % 2 ? -1.f : 1.f);
    }
    op[0] = op[n - 1] = -20.f;   // dead rows at both ends
    hc_mcmc_noise(n, xyz.data(), op.data(), sc.data(), rot.data(), nz.data(), 80.f);
    for (float v : xyz) sum += v;
    const float us[4] = {0.f, 0.99999994f, 0.5f, 1e-30f};
    for (int relocate = 0; relocate < 2; relocate++) {
        const int pos = hc_mcmc_weights(n, op.data(), 0.005f, relocate, w.data(), dead.data(), cdf.data(), idx.data());
        if (pos < 1) return 1;
        hc_mcmc_draw(pos, cdf.data(), idx.data(), cdf[pos - 1], 4, us, sampled.data());
        for (int k = 0; k < 4; k++) {
            bad += sampled[k] < 0 || sampled[k] >= n || !(w[sampled[k]] > 0.f);
            sum += sampled[k];
        }
    }
    hc_mcmc_relocate(n, op.data(), sc.data(), ratio.data(), 0.005f, no.data(), ns.data());
    for (int i = 0; i < n; i++) {
        if (ratio[i] < 2) continue;
        bad += !std::isfinite(no[i]) || !std::isfinite(ns[3 * i]) || !std::isfinite(ns[3 * i + 1]) || !std::isfinite(ns[3 * i + 2]);
        sum += no[i] + ns[3 * i];
    }
    for (int r = -1; r < 200; r++) bad += hc_mcmc_ratio_clamp(r) > r3::kMcmcMaxRatio;
    for (int nn = 0; nn < r3::kMcmcMaxRatio; nn++)
        for (int k = 0; k <= nn; k++) sum += hc_mcmc_binom(nn, k) * 1e-14;
    std::printf("checksum %.9g bad %d\n", sum, bad);
    return bad ? 1 : 0;
}
#endif
