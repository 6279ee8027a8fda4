// hostcheck_optim_rows.hip -- TEST SHIM: runs the per-lane logic of the visibility-gated Adam step
// (reduced-3dgs_amd/csrc/adam_math.h: the element-to-Gaussian mapping and the gated element, the __host__ __device__
// functions csrc/optim.hip's adam_visible_kernel calls) on the CPU, so tests/test_optim_visible_cpu.py can check them
// WITHOUT a GPU.  The walks below follow the kernel's: one chunk_origin per chunk of 1024 units, then 32-bit offsets.
// Not part of the product; nothing in reduced-3dgs_amd/ links it.
#include "../../reduced-3dgs_amd/csrc/adam_math.h"

namespace {
constexpr long long kChunkUnits = 1024;   // optim.hip: kBlock * kUnitsPerThread
}

extern "C" {

// x / row_len and x % row_len by the multiply-high and its fix-up
unsigned hc_row_divmod(int row_len, unsigned x, unsigned* rem) { return r3::row_divmod(r3::row_div(row_len), x, *rem); }

// Gaussian and remainder of element e0 (no memory is touched: e0 may be far past 2^31)
long long hc_chunk_origin(int row_len, long long e0, unsigned* rem)
{
    const r3::ChunkOrigin o = r3::chunk_origin(r3::row_div(row_len), e0);
    *rem = o.rem;
    return o.gaussian;
}

// The Gaussian of element e of a vector row [P, row_len] with `head` leading scalar floats, by the kernel's route: the
// head from 0, the tail from the end, a body element through its chunk's origin and its unit's walk.
long long hc_vector_row_gaussian(int row_len, long long P, int head, long long e)
{
    const r3::RowDiv d = r3::row_div(row_len);
    const long long n = P * row_len, units = (n - head) / 4, body_end = head + 4 * units;
    unsigned rem;
    if (e < head) return r3::row_divmod(d, (unsigned)e, rem);
    if (e >= body_end) return r3::tail_gaussian(d, P, (unsigned)(n - 1 - e));
    const long long u = (e - head) / 4, chunk = u / kChunkUnits;
    const r3::ChunkOrigin o = r3::chunk_origin(d, head + 4 * chunk * kChunkUnits);
    unsigned q[4];
    r3::unit_gaussians(d, o.rem, 4u * (unsigned)(u - chunk * kChunkUnits), q);
    return o.gaussian + q[(e - head) % 4];
}

// The same for a scalar row (a unit is one element)
long long hc_scalar_row_gaussian(int row_len, long long e)
{
    const r3::RowDiv d = r3::row_div(row_len);
    const long long chunk = e / kChunkUnits;
    const r3::ChunkOrigin o = r3::chunk_origin(d, chunk * kChunkUnits);
    unsigned rem;
    return o.gaussian + r3::element_gaussian(d, o.rem, (unsigned)(e - chunk * kChunkUnits), rem);
}

// One gated step of a vector row [P, row_len] with `head`, in place, as the kernel walks it: head and tail scalars, then
// float4 units; a unit without a visible element is not touched.  s[6] = w1, beta2, w2, bc2_sqrt, eps, step_size.
void hc_adam_step_visible(int row_len, long long P, int head, const int* radii, const float* s, const float* g, float* p,
                          float* m, float* v)
{
    const r3::AdamScalars sc{s[0], s[1], s[2], s[3], s[4], s[5]};
    const r3::RowDiv d = r3::row_div(row_len);
    const long long n = P * row_len, units = (n - head) / 4, body_end = head + 4 * units;
    unsigned rem;
    for (long long e = 0; e < head; e++)
        if (r3::gaussian_visible(radii[r3::row_divmod(d, (unsigned)e, rem)])) r3::adam_element(sc, g[e], p[e], m[e], v[e]);
    for (long long e = body_end; e < n; e++)
        if (r3::gaussian_visible(radii[r3::tail_gaussian(d, P, (unsigned)(n - 1 - e))]))
            r3::adam_element(sc, g[e], p[e], m[e], v[e]);
    for (long long u = 0; u < units; u++) {
        const long long chunk = u / kChunkUnits;
        const r3::ChunkOrigin o = r3::chunk_origin(d, head + 4 * chunk * kChunkUnits);
        unsigned q[4];
        r3::unit_gaussians(d, o.rem, 4u * (unsigned)(u - chunk * kChunkUnits), q);
        bool vis[4], any = false;
        for (int j = 0; j < 4; j++) any |= vis[j] = r3::gaussian_visible(radii[o.gaussian + q[j]]);
        if (!any) continue;
        const long long e = head + 4 * u;
        for (int j = 0; j < 4; j++) r3::adam_element_gated(sc, vis[j], g[e + j], p[e + j], m[e + j], v[e + j]);
    }
}

}  // extern "C"
