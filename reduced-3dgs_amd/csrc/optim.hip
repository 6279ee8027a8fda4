// optim.hip -- the fused Adam step of include/r3dgs_optim.h: every tensor of every parameter group in one launch.
//
// torch.optim.Adam's default step runs ~8 elementwise passes per group (lerp, mul, addcmul, sqrt, div, add, addcdiv and
// the step bump), about 72 B of traffic per parameter.  This kernel reads p, g, m, v and writes p, m, v once: 28 B.
//
// Segment table: up to kMaxRows tensors per launch, passed by value in the kernel arguments.  Each row is cut into chunks
// of kChunkUnits units (a unit is a float4 for a row whose four pointers share their 16-byte phase, else one float); the
// rows' chunks are numbered one after another and each 256-thread workgroup takes one chunk, finding its row by scanning
// the table's chunk_begin column.  A vector row's first 0-3 floats before the 16-byte boundary (head) and last 0-3
// (tail) are done with scalar code by the row's first chunk.  No LDS, no atomics, no allocation, no host synchronisation.
//
// Per element the arithmetic is adam_math.h's, compiled with -ffp-contract=off and correctly rounded divide/sqrt
// (build.py) so that the roundings it documents are exactly the ones executed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>

#include "adam_math.h"
#include "common.h"
#include "../../include/r3dgs_optim.h"

namespace {

constexpr int kBlock = 256;
constexpr int kUnitsPerThread = 4;                        // float4 units in flight per thread: 16 loads of 16 B
constexpr int kChunkUnits = kBlock * kUnitsPerThread;
constexpr int kMaxRows = R3DGS_ADAM_MAX_SEGMENTS;

// Common geometry of a row.  head >= 0: vector row, `head` scalar floats then `units` float4s then the tail; head < 0:
// scalar row, `units` == n floats.
struct RowGeom {
    float* p;
    const float* g;
    float* m;
    float* v;
    long long n;
    long long units;
    int chunk_begin;
    int head;
};

struct Row {
    RowGeom geo;
    r3::AdamScalars s;
};

struct CapRow {
    RowGeom geo;
    float* step;          // device step count, read here (+1) and bumped by adam_bump_kernel afterwards
    const float* lr;      // device lr or NULL
    double lr_value, beta1, beta2, eps;
};

template <class R>
struct Table {
    int rows;
    R r[kMaxRows];
};

__device__ inline r3::AdamScalars scalars_of(const Row& row) { return row.s; }

// Capturable: the bias corrections from the device step, in double, each rounded to fp32 once (as the host does).
__device__ inline r3::AdamScalars scalars_of(const CapRow& row)
{
    const double step = (double)(*row.step + 1.0f);   // the fp32 count after this step's bump
    const double lr = row.lr ? (double)*row.lr : row.lr_value;
    const double bc1 = 1.0 - pow(row.beta1, step);
    const double bc2 = 1.0 - pow(row.beta2, step);
    r3::AdamScalars s;
    s.w1 = (float)(1.0 - row.beta1);
    s.beta2 = (float)row.beta2;
    s.w2 = (float)(1.0 - row.beta2);
    s.bc2_sqrt = (float)sqrt(bc2);
    s.eps = (float)row.eps;
    s.step_size = (float)(-(lr / bc1));
    return s;
}

__device__ inline void scalar_element(const RowGeom& r, const r3::AdamScalars& s, long long e)
{
    float p = r.p[e], m = r.m[e], v = r.v[e];
    r3::adam_element(s, r.g[e], p, m, v);
    r.p[e] = p;
    r.m[e] = m;
    r.v[e] = v;
}

template <class R>
__global__ __launch_bounds__(kBlock) void adam_kernel(const Table<R> t)
{
    const int b = blockIdx.x;
    int ri = 0;
    while (ri + 1 < t.rows && t.r[ri + 1].geo.chunk_begin <= b) ri++;
    const R& row = t.r[ri];
    const RowGeom& geo = row.geo;
    const r3::AdamScalars s = scalars_of(row);
    const long long u0 = (long long)(b - geo.chunk_begin) * kChunkUnits + threadIdx.x;

    if (geo.head < 0) {   // scalar row: 4-byte loads, kUnitsPerThread in flight
        float g[kUnitsPerThread], p[kUnitsPerThread], m[kUnitsPerThread], v[kUnitsPerThread];
#pragma unroll
        for (int k = 0; k < kUnitsPerThread; k++) {
            const long long e = u0 + (long long)k * kBlock;
            if (e < geo.units) {
                g[k] = geo.g[e];
                p[k] = geo.p[e];
                m[k] = geo.m[e];
                v[k] = geo.v[e];
            }
        }
#pragma unroll
        for (int k = 0; k < kUnitsPerThread; k++) {
            const long long e = u0 + (long long)k * kBlock;
            if (e < geo.units) {
                r3::adam_element(s, g[k], p[k], m[k], v[k]);
                geo.p[e] = p[k];
                geo.m[e] = m[k];
                geo.v[e] = v[k];
            }
        }
        return;
    }

    // vector row: the head and the tail (each < 4 floats) by the first chunk's first lanes
    if (b == geo.chunk_begin) {
        const long long body_end = geo.head + 4 * geo.units;
        if ((int)threadIdx.x < geo.head) scalar_element(geo, s, threadIdx.x);
        else if (threadIdx.x >= 4 && threadIdx.x < 4 + (geo.n - body_end)) scalar_element(geo, s, body_end + threadIdx.x - 4);
    }
    const float4* g4 = reinterpret_cast<const float4*>(geo.g + geo.head);
    float4* p4 = reinterpret_cast<float4*>(geo.p + geo.head);
    float4* m4 = reinterpret_cast<float4*>(geo.m + geo.head);
    float4* v4 = reinterpret_cast<float4*>(geo.v + geo.head);
    float4 g[kUnitsPerThread], p[kUnitsPerThread], m[kUnitsPerThread], v[kUnitsPerThread];
#pragma unroll
    for (int k = 0; k < kUnitsPerThread; k++) {
        const long long u = u0 + (long long)k * kBlock;
        if (u < geo.units) {
            g[k] = g4[u];
            p[k] = p4[u];
            m[k] = m4[u];
            v[k] = v4[u];
        }
    }
#pragma unroll
    for (int k = 0; k < kUnitsPerThread; k++) {
        const long long u = u0 + (long long)k * kBlock;
        if (u < geo.units) {
            r3::adam_element(s, g[k].x, p[k].x, m[k].x, v[k].x);
            r3::adam_element(s, g[k].y, p[k].y, m[k].y, v[k].y);
            r3::adam_element(s, g[k].z, p[k].z, m[k].z, v[k].z);
            r3::adam_element(s, g[k].w, p[k].w, m[k].w, v[k].w);
            p4[u] = p[k];
            m4[u] = m[k];
            v4[u] = v[k];
        }
    }
}

// ---- the visibility-gated step (r3dgs_adam_step_visible*): adam_kernel's layout -- the same table, chunks, units, head and
// tail -- with every tensor a [P, row_len] array and only the Gaussians with radii > 0 updated.  Phase 1 loads the radii of
// the Gaussians a thread's units touch and waits once; phase 2 issues the 16-byte loads of g, p, m, v for the units with a
// visible element only, all in flight together.  A unit without a visible element is neither loaded nor stored; a partly
// visible one computes its four elements, keeps the old p, m, v of the culled ones by a select and stores the float4 whole.
template <class R>
struct VisibleTable {
    Table<R> t;
    r3::RowDiv div[kMaxRows];   // per row: row_len and its reciprocal
    const int* radii;           // int[P], read at run time (a captured graph follows the buffer's contents)
    long long P;
};

__device__ inline void scalar_element_visible(const RowGeom& r, const r3::AdamScalars& s, long long e, int radius)
{
    if (r3::gaussian_visible(radius)) scalar_element(r, s, e);
}

// Phase 1 of a vector row: bit j of vis[k] says that element j of the thread's k-th unit is visible.  A unit touches the
// Gaussians of its first and last element and, for rows shorter than 3 floats only (kTwo false), others in between.  Without
// a branch, so that all radii loads are issued before the one wait: a unit past the end reads the chunk's first unit's
// Gaussians (always there) and is masked out.
template <bool kTwo>
__device__ inline void unit_visibility(const r3::RowDiv& dv, unsigned origin_rem, const int* radii, long long u0,
                                       long long units, unsigned vis[kUnitsPerThread])
{
    int ra[kUnitsPerThread], rb[kUnitsPerThread], rc[kUnitsPerThread], rd[kUnitsPerThread];
    unsigned first[kUnitsPerThread];   // bit j: element j belongs to the Gaussian of element 0 (kTwo)
#pragma unroll
    for (int k = 0; k < kUnitsPerThread; k++) {
        const bool in = u0 + (long long)k * kBlock < units;
        unsigned q[4];
        r3::unit_gaussians(dv, origin_rem, in ? 4u * (threadIdx.x + k * kBlock) : 0u, q);
        ra[k] = radii[q[0]];
        rd[k] = radii[q[3]];
        if constexpr (kTwo) {
            first[k] = (q[1] == q[0] ? 2u : 0u) | (q[2] == q[0] ? 4u : 0u);
        } else {
            rb[k] = radii[q[1]];
            rc[k] = radii[q[2]];
        }
    }
#pragma unroll
    for (int k = 0; k < kUnitsPerThread; k++) {
        if constexpr (kTwo) {
            rb[k] = (first[k] & 2u) ? ra[k] : rd[k];
            rc[k] = (first[k] & 4u) ? ra[k] : rd[k];
        }
        const unsigned bits = (r3::gaussian_visible(ra[k]) ? 1u : 0u) | (r3::gaussian_visible(rb[k]) ? 2u : 0u) |
                              (r3::gaussian_visible(rc[k]) ? 4u : 0u) | (r3::gaussian_visible(rd[k]) ? 8u : 0u);
        vis[k] = u0 + (long long)k * kBlock < units ? bits : 0u;
    }
}

template <class R>
__global__ __launch_bounds__(kBlock) void adam_visible_kernel(const VisibleTable<R> vt)
{
    const Table<R>& t = vt.t;
    const int b = blockIdx.x;
    int ri = 0;
    while (ri + 1 < t.rows && t.r[ri + 1].geo.chunk_begin <= b) ri++;
    const R& row = t.r[ri];
    const RowGeom& geo = row.geo;
    const r3::RowDiv dv = vt.div[ri];
    const r3::AdamScalars s = scalars_of(row);
    const long long chunk_u0 = (long long)(b - geo.chunk_begin) * kChunkUnits;
    const long long u0 = chunk_u0 + threadIdx.x;

    if (geo.head < 0) {   // scalar row: a unit is one element of one Gaussian
        const r3::ChunkOrigin o = r3::chunk_origin(dv, chunk_u0);
        const int* radii = vt.radii + o.gaussian;
        int rad[kUnitsPerThread];
        float g[kUnitsPerThread], p[kUnitsPerThread], m[kUnitsPerThread], v[kUnitsPerThread];
        // phase 1, without a branch: a unit past the end reads the chunk's first Gaussian (always there) and is masked out
#pragma unroll
        for (int k = 0; k < kUnitsPerThread; k++) {
            const bool in = u0 + (long long)k * kBlock < geo.units;
            unsigned rem;
            rad[k] = radii[r3::element_gaussian(dv, o.rem, in ? threadIdx.x + k * kBlock : 0u, rem)];
        }
#pragma unroll
        for (int k = 0; k < kUnitsPerThread; k++) {
            if (u0 + (long long)k * kBlock >= geo.units) rad[k] = 0;
            asm volatile("" : "+v"(rad[k]));   // phase 1 ends here, as in the vector row below
        }
#pragma unroll
        for (int k = 0; k < kUnitsPerThread; k++) {
            const long long e = u0 + (long long)k * kBlock;
            if (r3::gaussian_visible(rad[k])) {
                g[k] = geo.g[e];
                p[k] = geo.p[e];
                m[k] = geo.m[e];
                v[k] = geo.v[e];
            }
        }
#pragma unroll
        for (int k = 0; k < kUnitsPerThread; k++) {
            const long long e = u0 + (long long)k * kBlock;
            if (r3::gaussian_visible(rad[k])) {
                r3::adam_element(s, g[k], p[k], m[k], v[k]);
                geo.p[e] = p[k];
                geo.m[e] = m[k];
                geo.v[e] = v[k];
            }
        }
        return;
    }

    // vector row: the head and the tail (each < 4 floats) by the first chunk's first lanes
    if (b == geo.chunk_begin) {
        const long long body_end = geo.head + 4 * geo.units;
        const long long tail = geo.n - body_end;
        if ((int)threadIdx.x < geo.head) {
            unsigned rem;
            scalar_element_visible(geo, s, threadIdx.x, vt.radii[r3::row_divmod(dv, threadIdx.x, rem)]);
        } else if (threadIdx.x >= 4 && threadIdx.x < 4 + tail) {
            const unsigned i = threadIdx.x - 4;   // the i-th tail element is the (tail - 1 - i)-th from the end
            scalar_element_visible(geo, s, body_end + i, vt.radii[r3::tail_gaussian(dv, vt.P, (unsigned)(tail - 1) - i)]);
        }
    }
    if (geo.units == 0) return;   // a tensor of head and tail only: from here on every chunk has a unit
    const r3::ChunkOrigin o = r3::chunk_origin(dv, geo.head + 4 * chunk_u0);
    const int* radii = vt.radii + o.gaussian;
    unsigned vis[kUnitsPerThread];
    if (dv.len >= 3) unit_visibility<true>(dv, o.rem, radii, u0, geo.units, vis);
    else unit_visibility<false>(dv, o.rem, radii, u0, geo.units, vis);
    // phase 1 ends here: every unit's bits are in registers before the first load of phase 2 is issued (left to itself
    // the compiler sinks the last unit's bits, and their wait on the radii, below the other units' loads)
#pragma unroll
    for (int k = 0; k < kUnitsPerThread; k++) asm volatile("" : "+v"(vis[k]));
    // phase 2
    const float4* g4 = reinterpret_cast<const float4*>(geo.g + geo.head);
    float4* p4 = reinterpret_cast<float4*>(geo.p + geo.head);
    float4* m4 = reinterpret_cast<float4*>(geo.m + geo.head);
    float4* v4 = reinterpret_cast<float4*>(geo.v + geo.head);
    float4 g[kUnitsPerThread], p[kUnitsPerThread], m[kUnitsPerThread], v[kUnitsPerThread];
#pragma unroll
    for (int k = 0; k < kUnitsPerThread; k++) {
        const long long u = u0 + (long long)k * kBlock;
        if (vis[k]) {
            g[k] = g4[u];
            p[k] = p4[u];
            m[k] = m4[u];
            v[k] = v4[u];
        }
    }
#pragma unroll
    for (int k = 0; k < kUnitsPerThread; k++) {
        const long long u = u0 + (long long)k * kBlock;
        if (vis[k]) {
            r3::adam_element_gated(s, vis[k] & 1u, g[k].x, p[k].x, m[k].x, v[k].x);
            r3::adam_element_gated(s, vis[k] & 2u, g[k].y, p[k].y, m[k].y, v[k].y);
            r3::adam_element_gated(s, vis[k] & 4u, g[k].z, p[k].z, m[k].z, v[k].z);
            r3::adam_element_gated(s, vis[k] & 8u, g[k].w, p[k].w, m[k].w, v[k].w);
            p4[u] = p[k];
            m4[u] = m[k];
            v4[u] = v[k];
        }
    }
}

// Capturable mode, after adam_kernel on the same stream: step[0] += 1 for each row.
__global__ void adam_bump_kernel(const Table<CapRow> t)
{
    const int i = threadIdx.x;
    if (i < t.rows) *t.r[i].step = *t.r[i].step + 1.0f;
}

// Fills the geometry of a row; returns its chunk count (0 for an empty tensor).
int fill_geom(RowGeom& geo, float* p, const float* g, float* m, float* v, long long n, int chunk_begin, int index)
{
    const std::string where = "adam: segment " + std::to_string(index);
    if (n < 0) throw r3::Error(where + ": negative element count");
    if (n > 0 && (!p || !g || !m || !v)) throw r3::Error(where + ": a pointer is NULL");
    const uintptr_t a[4] = {(uintptr_t)p, (uintptr_t)g, (uintptr_t)m, (uintptr_t)v};
    for (uintptr_t x : a)
        if (x % 4) throw r3::Error(where + ": a pointer is not 4-byte aligned");
    geo.p = p;
    geo.g = g;
    geo.m = m;
    geo.v = v;
    geo.n = n;
    geo.chunk_begin = chunk_begin;
    const uintptr_t phase = (a[0] / 4) % 4;
    const bool vec = (a[1] / 4) % 4 == phase && (a[2] / 4) % 4 == phase && (a[3] / 4) % 4 == phase;
    if (vec) {
        const long long head = std::min<long long>(n, (long long)((4 - phase) % 4));
        geo.head = (int)head;
        geo.units = (n - head) / 4;
    } else {
        geo.head = -1;
        geo.units = n;
    }
    if (n == 0) return 0;
    const long long chunks = std::max<long long>(1, (geo.units + kChunkUnits - 1) / kChunkUnits);
    if (chunks > (1LL << 30)) throw r3::Error(where + ": too many elements");
    return (int)chunks;
}

// Row fillers of the two segment kinds: the row's scalars or device pointers, then its geometry (fill_geom's chunk count).
int fill_row(Row& row, const r3dgs_adam_segment& sg, int chunk_begin, int index)
{
    row.s = {sg.lerp_weight, sg.beta2, sg.addcmul_value, sg.bc2_sqrt, sg.eps, sg.step_size};
    return fill_geom(row.geo, sg.param, sg.grad, sg.exp_avg, sg.exp_avg_sq, sg.n, chunk_begin, index);
}

int fill_row(CapRow& row, const r3dgs_adam_capturable_segment& sg, int chunk_begin, int index)
{
    if (!sg.step) throw r3::Error("adam (capturable): segment " + std::to_string(index) + ": step is NULL");
    row.step = sg.step;
    row.lr = sg.lr;
    row.lr_value = sg.lr_value;
    row.beta1 = sg.beta1;
    row.beta2 = sg.beta2;
    row.eps = sg.eps;
    return fill_geom(row.geo, sg.param, sg.grad, sg.exp_avg, sg.exp_avg_sq, sg.n, chunk_begin, index);
}

// The visibility arguments of a gated step; row_len == nullptr is the dense step.
struct Visible {
    const int* row_len = nullptr;
    const int* radii = nullptr;
    long long P = 0;
};

template <class Seg, class R>
void run_batches(int n_segments, const Seg* segments, hipStream_t stream, const Visible& vis = {})
{
    constexpr bool bump = std::is_same<R, CapRow>::value;
    if (n_segments < 0) throw r3::Error("adam: negative segment count");
    if (n_segments > 0 && !segments) throw r3::Error("adam: segments is NULL");
    if (vis.row_len) {   // every refusal of the gated step comes before its first launch
        if (vis.P < 0) throw r3::Error("adam (visible): negative Gaussian count");
        if (vis.P > 0 && !vis.radii) throw r3::Error("adam (visible): radii is NULL");
        if ((uintptr_t)vis.radii % 4) throw r3::Error("adam (visible): radii is not 4-byte aligned");
        for (int i = 0; i < n_segments; i++) {
            const std::string where = "adam (visible): segment " + std::to_string(i);
            if (vis.row_len[i] < 1) throw r3::Error(where + ": row_len " + std::to_string(vis.row_len[i]) + " < 1");
            long long want;
            if (__builtin_mul_overflow(vis.P, (long long)vis.row_len[i], &want) || segments[i].n != want)
                throw r3::Error(where + ": n " + std::to_string(segments[i].n) + " is not P * row_len = " +
                                std::to_string(vis.P) + " * " + std::to_string(vis.row_len[i]));
            R probe{};
            fill_row(probe, segments[i], 0, i);
        }
    }
    int i = 0;
    while (i < n_segments) {
        VisibleTable<R> vt{};
        Table<R>& t = vt.t;
        int rows = 0;
        long long chunks = 0;
        for (; i < n_segments && rows < kMaxRows; i++) {
            R& row = t.r[rows];
            const int c = fill_row(row, segments[i], (int)chunks, i);
            if (c == 0 && !bump) continue;   // an empty tensor: nothing to do (capturable: its step is still bumped)
            if (vis.row_len) vt.div[rows] = r3::row_div(vis.row_len[i]);
            chunks += c;
            if (chunks >= (1LL << 31)) throw r3::Error("adam: too many elements in one launch");
            rows++;
        }
        t.rows = rows;
        if (rows == 0) break;
        if (chunks > 0) {
            if (vis.row_len) {
                vt.radii = vis.radii;
                vt.P = vis.P;
                adam_visible_kernel<R><<<(unsigned)chunks, kBlock, 0, stream>>>(vt);
            } else {
                adam_kernel<R><<<(unsigned)chunks, kBlock, 0, stream>>>(t);
            }
            r3::check_launch("adam step", stream, false);
        }
        if constexpr (bump) {
            adam_bump_kernel<<<1, 64, 0, stream>>>(t);
            r3::check_launch("adam step bump", stream, false);
        }
    }
}

}  // namespace

extern "C" {

int r3dgs_adam_step(int n_segments, const r3dgs_adam_segment* segments, void* stream)
{
    return r3::guarded_call([&]() {
        run_batches<r3dgs_adam_segment, Row>(n_segments, segments, static_cast<hipStream_t>(stream));
        return 0;
    });
}

int r3dgs_adam_step_capturable(int n_segments, const r3dgs_adam_capturable_segment* segments, void* stream)
{
    return r3::guarded_call([&]() {
        run_batches<r3dgs_adam_capturable_segment, CapRow>(n_segments, segments, static_cast<hipStream_t>(stream));
        return 0;
    });
}

int r3dgs_adam_step_visible(int n_segments, const r3dgs_adam_segment* segments, const int* row_len, const int* radii,
                            long long P, void* stream)
{
    return r3::guarded_call([&]() {
        if (!row_len && n_segments > 0) throw r3::Error("adam (visible): row_len is NULL");
        const int one = 1;   // no segments: nothing to check per row
        run_batches<r3dgs_adam_segment, Row>(n_segments, segments, static_cast<hipStream_t>(stream),
                                             {row_len ? row_len : &one, radii, P});
        return 0;
    });
}

int r3dgs_adam_step_capturable_visible(int n_segments, const r3dgs_adam_capturable_segment* segments, const int* row_len,
                                       const int* radii, long long P, void* stream)
{
    return r3::guarded_call([&]() {
        if (!row_len && n_segments > 0) throw r3::Error("adam (visible): row_len is NULL");
        const int one = 1;
        run_batches<r3dgs_adam_capturable_segment, CapRow>(n_segments, segments, static_cast<hipStream_t>(stream),
                                                           {row_len ? row_len : &one, radii, P});
        return 0;
    });
}

}  // extern "C"
