// preprocess.hip -- per-view, per-Gaussian forward stage on gfx950 (wave64).
//
// Replaces cuda_rasterizer/forward.cu:353-456 preprocessCUDA (dense SH [P,M,3] + per-Gaussian degrees),
// forward.cu:245-350 variableSHPreprocessCUDA (ragged degree-sorted SH buffer) and
// rasterizer_impl.cu:62-74 checkFrustum of /root/reference/submodules/diff-gaussian-rasterization.
//
// One lane per Gaussian, 256-thread workgroups, two roles: geometry (everything the binning needs; its sort keys go
// to the depth sort at once -- this kernel also installs the pass block, its by-value argument) and colour (the
// HBM-heavy SH stream, which rides in spare workgroups of the three depth-sort launches so that it runs underneath
// that sort inside one linear launch chain).  In the colour role each wave first copies the SH rows of
// its 64 Gaussians -- one contiguous span of the [P,M,3] tensor (or of the ragged buffer) -- into LDS with
// fully coalesced loads, then every lane evaluates its own row out of LDS (bank-skewed index), instead of 64
// lanes striding 192 B apart through global memory.  Output is one 48-byte record per visible Gaussian (GRec),
// the tile rect, the depth sort key and tiles_touched.
// Built with -ffp-contract=off: radii / rects / tiles_touched are bit-exact against the oracle.
#include <cstdlib>
#include <map>
#include <mutex>

#include "depth_sort.h"
#include "quant_math.h"
#include "sh_rows.h"

namespace r3 {

constexpr int kPreBlock = kPreBlockSize;

// chunks of BLOCK Gaussians (one round of a workgroup of the geometry kernel or of a colour role) that cover P
template <int BLOCK = kPreBlock>
__host__ __device__ constexpr int pre_chunks(int P)
{
    return (P + BLOCK - 1) / BLOCK;
}

// ---- kernel 1: geometry ---------------------------------------------------------------------------
// cull, projection, conic, radius, tile rect, depth key, per-view counters.  Reads 44 B per Gaussian.  Its
// outputs are everything the depth sort / binning needs, so the SH -> RGB stream can ride in spare workgroups of
// the (launch-latency-bound) sort's kernels.
// COLOR is 0, or 4 (r3dgs_forward_params): scales / rotations hold the model's RAW parameters and are activated after the
// load (param_math.h).  The two keep these numbers because the committed profiles and bench.py cite the kernels by name.
// COLOR 5 (r3dgs_quantised_forward): the raw parameters are looked up from the codebooks (quant_math.h; 8 id bytes and 6 or
// 12 position bytes per Gaussian, the four geometry codebooks -- 4 KB -- through the cache), then activated as for 4.
template <int COLOR>
__global__ __launch_bounds__(kPreBlock) void preprocess_geom_kernel(FwdPassArgs* dst, FwdPassArgs v)
{
    static_assert(COLOR == 0 || COLOR == 4 || COLOR == 5, "0: activated inputs, 4: raw parameters, 5: codebook ids");
    // first kernel of the forward: it gets the pass block by value, installs it for the kernels behind it ...
    if (blockIdx.x == 0) install_block_from_kernarg(dst, (int)threadIdx.x, kPreBlock);
    const PreArgs a = v.pre;   // ... and reads its own arguments from the kernarg segment (scalar loads)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = a.in.P;
    const int i = blockIdx.x * kPreBlock + tid;
    const bool valid = i < P;
    const Camera cam = load_camera(a.view);

    PreOut o;
    o.radius = 0;
    o.tiles = 0;
    o.tiles_ref = 0;
    o.depth = 0.f;
    if (COLOR == 5) {
        if (valid) {
            float m[3], raw_op, sc[3], rq[4], q[4];
            quant_xyz(v.quant.xyz, v.quant.xyz_is_half, i, m);
            const uint2 gw = reinterpret_cast<const uint2*>(v.quant.geom_ids)[i];   // the eight ids in one load
            const uint8_t gid[8] = {(uint8_t)gw.x, (uint8_t)(gw.x >> 8), (uint8_t)(gw.x >> 16), (uint8_t)(gw.x >> 24),
                                    (uint8_t)gw.y, (uint8_t)(gw.y >> 8), (uint8_t)(gw.y >> 16), (uint8_t)(gw.y >> 24)};
            quant_geom(v.quant.codebooks, gid, &raw_op, sc, rq);
            for (int k = 0; k < 3; k++) sc[k] = scale_act(sc[k]);
            quat_act(rq, q);
            preprocess_one(cam, m[0], m[1], m[2], sc, q, nullptr, raw_op, &o, a.tight != 0);
        }
    } else if (valid) {
        const float mx = a.in.means3D[3 * i], my = a.in.means3D[3 * i + 1], mz = a.in.means3D[3 * i + 2];
        float sc[3] = {0.f, 0.f, 0.f}, q[4] = {1.f, 0.f, 0.f, 0.f}, c6[6];
        const float* c6p = nullptr;
        if (a.in.cov3D_precomp) {
            for (int k = 0; k < 6; k++) c6[k] = a.in.cov3D_precomp[6 * i + k];
            c6p = c6;
        } else {
            for (int k = 0; k < 3; k++) sc[k] = a.in.scales[3 * i + k];
            const float4 qv = reinterpret_cast<const float4*>(a.in.rotations)[i];
            q[0] = qv.x;
            q[1] = qv.y;
            q[2] = qv.z;
            q[3] = qv.w;
            if (COLOR == 4) {
                const float rq[4] = {q[0], q[1], q[2], q[3]};
                for (int k = 0; k < 3; k++) sc[k] = scale_act(sc[k]);
                quat_act(rq, q);
            }
        }
        preprocess_one(cam, mx, my, mz, sc, q, c6p, a.in.opacities[i], &o, a.tight != 0);
    }
    if (valid) {
        uint32_t dkey = 0xFFFFFFFFu;
        if (o.radius > 0) {
            GRec r;
            r.x = o.px;
            r.y = o.py;
            r.cA = o.conic[0];
            r.cB = o.conic[1];
            r.cC = o.conic[2];
            r.op = o.opacity;
            r.r = r.g = r.b = 0.f;  // filled in by the colour kernel
            r.rect_min = (uint32_t)o.rmin[0] | ((uint32_t)o.rmin[1] << 16);
            r.width_clamp = (uint32_t)(o.rmax[0] - o.rmin[0]);  // clamp bits OR-ed in by the colour kernel
            r.pair_start = 0xFFFFFFFFu;   // filled in by the pair-emission kernel (stays ~0 if no pair was emitted)
            a.rec[i] = r;
            a.rect[i] = make_ushort4((unsigned short)o.rmin[0], (unsigned short)o.rmin[1], (unsigned short)o.rmax[0],
                                     (unsigned short)o.rmax[1]);
            // a visible Gaussian whose opacity-aware rect is empty owns no pair: it stays out of the depth order like a
            // culled one (its radius, record and gradients are those of a visible Gaussian)
            if (o.tiles > 0) dkey = __float_as_uint(o.depth);
        }
        a.radii[i] = o.radius;
        a.tiles[i] = o.tiles;
        a.depth_key[i] = dkey;
    }
    // per-workgroup totals, stored (not accumulated): visible count (SH-sparsity normaliser of the backward),
    // num_rendered, and the depth range of the visible Gaussians (bucketed depth sort, binning.hip).  R does not depend
    // on the depth order, so the host can fetch it while the GPU is busy with the depth sort (pass_driver.hip forward_exact).
    const unsigned long long vmask = __ballot(o.radius > 0);
    const bool binned = o.tiles > 0;
    const unsigned long long bmask = __ballot(binned);
    uint32_t tsum = o.tiles, rsum = o.tiles_ref;
    uint32_t dmax = binned ? __float_as_uint(o.depth) : 0u, dinv = binned ? ~__float_as_uint(o.depth) : 0u;
    for (int off = 32; off > 0; off >>= 1) {
        tsum += (uint32_t)__shfl_xor((int)tsum, off);
        rsum += (uint32_t)__shfl_xor((int)rsum, off);
        dmax = max(dmax, (uint32_t)__shfl_xor((int)dmax, off));
        dinv = max(dinv, (uint32_t)__shfl_xor((int)dinv, off));
    }
    __shared__ uint32_t s_cnt[kPreBlock / 64][6];
    if (lane == 0) {
        s_cnt[wave][0] = (uint32_t)__popcll(vmask);
        s_cnt[wave][1] = tsum;
        s_cnt[wave][2] = dmax;
        s_cnt[wave][3] = dinv;
        s_cnt[wave][4] = (uint32_t)__popcll(bmask);
        s_cnt[wave][5] = rsum;
    }
    __syncthreads();
    if (tid == 0) {
        PrePartial pp = {0u, 0u, 0u, 0u, 0u, 0u, {0u, 0u}};
        for (int k = 0; k < kPreBlock / 64; k++) {
            pp.visible += s_cnt[k][0];
            pp.num_rendered += s_cnt[k][1];
            pp.depth_max = max(pp.depth_max, s_cnt[k][2]);
            pp.depth_inv_min = max(pp.depth_inv_min, s_cnt[k][3]);
            pp.binned += s_cnt[k][4];
            pp.rendered_ref += s_cnt[k][5];
        }
        a.partials[blockIdx.x] = pp;
    }
}

// ---- kernel 2: colour -------------------------------------------------------------------------------
// SH -> RGB (forward.cu:105-159, ragged variant :19-100) or copy of the precomputed colours into the
// records of the visible Gaussians.  Streams the SH tensor (192 B per Gaussian at degree 3): the wave's 64 rows
// are one contiguous span, staged through LDS with dwordx4 loads, evaluated per lane from LDS (sh_rows.h: the layout, the
// row accessor and the staging; twelve loads per lane in flight).
// Launched as a SMALL persistent grid (issue_preprocess_color): the kernel is bandwidth-bound filler next to the
// latency-bound depth-sort kernels of the main stream, and a full grid's LDS footprint (3 x 49 KB per CU) left their
// workgroups no room -- the depth scatter kernel took 46 us instead of 14 us beside it.
constexpr size_t kColorLds = sizeof(float) * (kPreBlock / 64) * kWaveShFloats;

// the colour roles' epilogue: rgb and the clamp bits into the record of a visible Gaussian
__device__ __forceinline__ void store_color(GRec* r, const float* rgb, uint32_t cbits)
{
    r->r = rgb[0];
    r->g = rgb[1];
    r->b = rgb[2];
    if (cbits) r->width_clamp |= cbits << 16;  // same lane wrote the width in the geometry kernel
}

// chunks [first + wg, last) in steps of n_wg, BLOCK Gaussians each (BLOCK = workgroup size, always kPreBlock); smem: BLOCK / 64
// wave windows.
// SPLIT: the rows come from two tensors, in.shs = features_dc and shs_rest (sh_rows.h stage_split_rows); the LDS layout is the same.
template <bool RAGGED, int BLOCK, bool SPLIT = false>
__device__ __forceinline__ void color_role(const PreArgs& a, char* smem, int first, int last, int wg, int n_wg,
                                           const float* shs_rest = nullptr)
{
    float(*s_sh)[kWaveShFloats] = reinterpret_cast<float(*)[kWaveShFloats]>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = a.in.P, M = a.in.M;
    const bool rows48 = !RAGGED && M == 16;   // dense degree-3 tensor (wave-uniform)
  for (int blk = first + wg; blk < last; blk += n_wg) {
    const int i = blk * BLOCK + tid;
    const bool valid = i < P;
    const int wave_first = blk * BLOCK + wave * 64;
    const bool vis = valid && a.tiles[i] > 0;
    const bool need_sh = vis && (a.in.colors_precomp == nullptr);

    // ---- per-lane SH row placement inside the wave's contiguous span --------------------------
    int deg = 0, roff = 0;  // roff in floats relative to the span start
    long span_first = 0;    // first float of the wave's span in the SH buffer
    int span_len = 0;       // floats
    if (a.in.colors_precomp == nullptr) {
        if (RAGGED) {
            const int last_i = min(wave_first + 63, P - 1);
            int d0, dl;
            const int off_first = wave_first < P ? quant_ragged_offset(wave_first, a.in.coeffs_num, a.in.per_band_count, a.in.cumsum_count, &d0) : 0;
            const int off_last = wave_first < P ? quant_ragged_offset(last_i, a.in.coeffs_num, a.in.per_band_count, a.in.cumsum_count, &dl) : 0;
            span_first = 3L * off_first;
            span_len = wave_first < P ? 3 * (off_last + (dl + 1) * (dl + 1) - off_first) : 0;
            if (valid) {
                const int off = quant_ragged_offset(i, a.in.coeffs_num, a.in.per_band_count, a.in.cumsum_count, &deg);
                roff = 3 * (off - off_first);
            }
        } else {
            const int nrows = max(0, min(64, P - wave_first));
            span_first = 3L * M * wave_first;
            span_len = nrows * 3 * M;
            roff = lane * 3 * M;
            if (valid) deg = a.in.degrees[i];
        }
    }
    // wave-uniform: does any lane of this wave need its SH row?
    const bool wave_needs = __ballot(need_sh) != 0ull;
    if (SPLIT) {
        if (wave_needs) {
            const int nrows = max(0, min(64, P - wave_first));
            if (rows48)
                stage_split_rows<true>(a.in.shs, shs_rest, wave_first, nrows, M, s_sh[wave], lane);
            else
                stage_split_rows<false>(a.in.shs, shs_rest, wave_first, nrows, M, s_sh[wave], lane);
        }
    } else if (wave_needs) {   // twelve loads per lane cover a full degree-3 span (64 rows x 192 B)
        stage_span<12>(a.in.shs, span_first, span_len, rows48, s_sh[wave], lane);
    }
    __syncthreads();

    if (vis) {
        float rgb[3];
        uint32_t cbits = 0;
        if (need_sh) {
            const float campos[3] = {a.view.campos[0], a.view.campos[1], a.view.campos[2]};
            const float mx = a.in.means3D[3 * i], my = a.in.means3D[3 * i + 1], mz = a.in.means3D[3 * i + 2];
            // the colour, and -- while the row is here -- its derivatives with respect to the view direction, which is all
            // the backward wants from the row (GeomState::sh_ddir)
            auto eval = [&](const auto& row) {
                sh_to_rgb(deg, row, mx, my, mz, campos, rgb, &cbits);
                if (!RAGGED && a.sh_ddir && deg > 0) {
                    float d9[9];
                    sh_dir_derivs_at(deg, row, mx, my, mz, campos, d9);
                    float* o = a.sh_ddir + 9 * (size_t)i;
#pragma unroll
                    for (int k = 0; k < 9; k++) o[k] = d9[k];
                }
            };
            if (rows48)
                eval(sh_row<true, const float>(s_sh[wave], lane, roff));
            else
                eval(sh_row<false, const float>(s_sh[wave], lane, roff));
        } else {
            rgb[0] = a.in.colors_precomp[3 * i];
            rgb[1] = a.in.colors_precomp[3 * i + 1];
            rgb[2] = a.in.colors_precomp[3 * i + 2];
        }
        store_color(a.rec + i, rgb, cbits);
    }
    __syncthreads();   // the staging buffer is reused by the next round
  }
}

// ---- colour role over the quantised model (r3dgs_quantised_forward) ---------------------------------------------------
// The wave's 64 rows are one contiguous BYTE span of sh_ids (at most 64 x 48 B).  It starts at 3 * off_first bytes, which
// is in general not aligned: the wave copies the 16-byte chunks that cover the span, aligned by ADDRESS, into LDS with
// dwordx4 loads; a chunk that reaches in front of the array's first byte or behind its last (at most the first and the
// last chunk of a span at an end of the array) is put together from byte loads of the bytes that exist.  The sixteen SH
// codebooks (16 KB) are copied into LDS once per workgroup; a lane evaluates sh_to_rgb through an accessor that reads an id
// byte of its row and gathers the centre -- the same values in the same order as the fp32 ragged path reads from its row.
// LDS words of the id window are skewed one per 32 like the fp32 rows (lanes of a degree read 3 / 12 / 27 / 48 B apart).
constexpr int kQuantSpanChunks = (64 * kShRowFloats + 15 + 15) / 16 + 1;                 // 16-byte chunks of a misaligned span
constexpr int kQuantSpanWords = 4 * kQuantSpanChunks + (4 * kQuantSpanChunks) / 32 + 1;   // + skew
constexpr size_t kQuantBooksLds = sizeof(float) * kQuantShBooks * kQuantCentres;
constexpr size_t kQuantColorLds = kQuantBooksLds + sizeof(uint32_t) * (kPreBlock / 64) * kQuantSpanWords;
static_assert(kQuantSpanChunks <= 4 * 64, "four chunks per lane cover a span");

struct ShRowQuantLds {
    const uint8_t* ids;   // the wave's id window (skewed words)
    int roff;             // first byte of the lane's row in the window
    const float* books;   // [16][256] in LDS
    __device__ __forceinline__ float at(int e) const
    {
        const int b = roff + e, w = b >> 2;
        const uint32_t id = ids[(sh_skew<false>(w) << 2) | (b & 3)];
        return books[(quant_sh_book(e) << 8) + (int)id];
    }
};

template <int BLOCK>
__device__ __forceinline__ void color_role_quant(const PreArgs& a, const QuantInputs& qi, char* smem, int first, int last, int wg,
                                                 int n_wg)
{
    float* s_books = reinterpret_cast<float*>(smem);
    uint32_t(*s_ids)[kQuantSpanWords] = reinterpret_cast<uint32_t(*)[kQuantSpanWords]>(smem + kQuantBooksLds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = a.in.P;
    if (first + wg < last) {   // (the first barrier of the loop below orders these stores in front of every read)
        const float4* src = reinterpret_cast<const float4*>(qi.codebooks);
        for (int k = tid; k < kQuantShBooks * kQuantCentres / 4; k += BLOCK) reinterpret_cast<float4*>(s_books)[k] = src[k];
    }
    const uintptr_t arr_begin = reinterpret_cast<uintptr_t>(qi.sh_ids);
    const uintptr_t arr_end = arr_begin + (uintptr_t)quant_sh_bytes(a.in.coeffs_num, a.in.per_band_count);
  for (int blk = first + wg; blk < last; blk += n_wg) {
    const int i = blk * BLOCK + tid;
    const bool valid = i < P;
    const int wave_first = blk * BLOCK + wave * 64;
    const bool vis = valid && a.tiles[i] > 0;

    int deg = 0, roff = 0;
    uintptr_t win = 0;   // address of the first chunk
    int nchunks = 0;
    if (wave_first < P) {
        const int last_i = min(wave_first + 63, P - 1);
        int d0, dl;
        const int off_first = quant_ragged_offset(wave_first, a.in.coeffs_num, a.in.per_band_count, a.in.cumsum_count, &d0);
        const int off_last = quant_ragged_offset(last_i, a.in.coeffs_num, a.in.per_band_count, a.in.cumsum_count, &dl);
        const uintptr_t span = arr_begin + 3ull * (uintptr_t)off_first;
        const int span_len = 3 * (off_last + (dl + 1) * (dl + 1) - off_first);
        const int head = (int)(span & 15u);
        win = span - (uintptr_t)head;
        nchunks = (head + span_len + 15) >> 4;
        if (valid) {
            const int off = quant_ragged_offset(i, a.in.coeffs_num, a.in.per_band_count, a.in.cumsum_count, &deg);
            roff = head + 3 * (off - off_first);
        }
    }
    if (__ballot(vis) != 0ull) {
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = k * 64 + lane;
            v[k] = make_uint4(0u, 0u, 0u, 0u);
            if (c < nchunks) {
                const uintptr_t p = win + 16ull * (uintptr_t)c;
                if (p >= arr_begin && p + 16 <= arr_end) {
                    v[k] = *reinterpret_cast<const uint4*>(p);
                } else {   // an end of the array: only the bytes that exist
                    uint32_t w[4] = {0u, 0u, 0u, 0u};
                    for (int b = 0; b < 16; b++) {
                        const uintptr_t q = p + (uintptr_t)b;
                        if (q >= arr_begin && q < arr_end) w[b >> 2] |= (uint32_t)(*reinterpret_cast<const uint8_t*>(q)) << (8 * (b & 3));
                    }
                    v[k] = make_uint4(w[0], w[1], w[2], w[3]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = k * 64 + lane;
            if (c < nchunks) {
                const int w = 4 * c;   // four words of one chunk never straddle a skew step: 4 c % 32 <= 28
                uint32_t* d = s_ids[wave] + w + (w >> 5);   // word sh_skew<false>(w)
                d[0] = v[k].x;
                d[1] = v[k].y;
                d[2] = v[k].z;
                d[3] = v[k].w;
            }
        }
    }
    __syncthreads();

    if (vis) {
        float rgb[3], m[3];
        uint32_t cbits = 0;
        const float campos[3] = {a.view.campos[0], a.view.campos[1], a.view.campos[2]};
        quant_xyz(qi.xyz, qi.xyz_is_half, i, m);
        sh_to_rgb(deg, ShRowQuantLds{reinterpret_cast<const uint8_t*>(s_ids[wave]), roff, s_books}, m[0], m[1], m[2], campos, rgb,
                  &cbits);
        store_color(a.rec + i, rgb, cbits);
    }
    __syncthreads();   // the id window is reused by the next round
  }
}

// standalone colour kernel (generic depth sort path only): small persistent grid
template <bool RAGGED, int BLOCK>
__global__ __launch_bounds__(BLOCK) void preprocess_color_kernel(const PreArgs* __restrict__ ap)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PreArgs a = *ap;
    color_role<RAGGED, BLOCK>(a, smem, 0, pre_chunks<BLOCK>(a.in.P), (int)blockIdx.x, (int)gridDim.x);
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void preprocess_color_params_kernel(const FwdPassArgs* __restrict__ pa)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PreArgs a = pa->pre;
    color_role<false, BLOCK, true>(a, smem, 0, pre_chunks<BLOCK>(a.in.P), (int)blockIdx.x, (int)gridDim.x, pa->shs_rest);
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void preprocess_color_quant_kernel(const FwdPassArgs* __restrict__ pa)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PreArgs a = pa->pre;
    const QuantInputs qi = pa->quant;
    color_role_quant<BLOCK>(a, qi, smem, 0, pre_chunks<BLOCK>(a.in.P), (int)blockIdx.x, (int)gridDim.x);
}

// ---- depth-sort kernels carrying a share of the colour stream in extra workgroups -------------------------------
// Workgroups [0, n_sort) run the depth-sort role, workgroups [n_sort, n_sort + n_color) the colour chunks
// [c0, c1).  One dynamic LDS window serves whichever role a workgroup has.
// the sort role of launch STEP: histogram, scatter, bucket sort
template <int STEP>
__device__ __forceinline__ void depth_sort_role(const FwdPassArgs* __restrict__ pa, char* smem, int wg, int n_sort)
{
    const DepthArgs d = pa->depth;
    if (STEP == 0)
        depth_hist_role(d, pa->header, smem, wg);
    else if (STEP == 1)
        depth_scatter_role(d, smem, wg);
    else
        depth_bucket_group_role(d, smem, wg, n_sort);
}

template <int STEP, bool RAGGED>
__global__ __launch_bounds__(kPreBlock) void depth_sort_color_kernel(const FwdPassArgs* __restrict__ pa, int n_sort,
                                                                     int c0, int c1)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wg = (int)blockIdx.x;
    if (wg < n_sort) {
        depth_sort_role<STEP>(pa, smem, wg, n_sort);
    } else {
        const PreArgs a = pa->pre;
        color_role<RAGGED, kPreBlock>(a, smem, c0, c1, wg - n_sort, (int)gridDim.x - n_sort);
    }
}

// the same with the colour role reading the two SH tensors of the raw-parameter entry
template <int STEP>
__global__ __launch_bounds__(kPreBlock) void depth_sort_color_params_kernel(const FwdPassArgs* __restrict__ pa, int n_sort,
                                                                            int c0, int c1)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wg = (int)blockIdx.x;
    if (wg < n_sort) {
        depth_sort_role<STEP>(pa, smem, wg, n_sort);
    } else {
        const PreArgs a = pa->pre;
        color_role<false, kPreBlock, true>(a, smem, c0, c1, wg - n_sort, (int)gridDim.x - n_sort, pa->shs_rest);
    }
}

// the same with the colour role reading the quantised model
template <int STEP>
__global__ __launch_bounds__(kPreBlock) void depth_sort_color_quant_kernel(const FwdPassArgs* __restrict__ pa, int n_sort,
                                                                           int c0, int c1)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wg = (int)blockIdx.x;
    if (wg < n_sort) {
        depth_sort_role<STEP>(pa, smem, wg, n_sort);
    } else {
        const PreArgs a = pa->pre;
        const QuantInputs qi = pa->quant;
        color_role_quant<kPreBlock>(a, qi, smem, c0, c1, wg - n_sort, (int)gridDim.x - n_sort);
    }
}

__global__ __launch_bounds__(64 * kColWaves) void depth_colscan_kernel(const DepthArgs* __restrict__ ap)
{
    const DepthArgs d = *ap;
    depth_colscan_role(d, (int)blockIdx.x);
}

void issue_preprocess_geom(const FwdPlan& p, FwdPassArgs* dst, const FwdPassArgs& v, hipStream_t s)
{
    const int blocks = pre_chunks(p.P);
    if (p.quant)
        hipLaunchKernelGGL(preprocess_geom_kernel<5>, dim3(blocks), dim3(kPreBlock), 0, s, dst, v);
    else if (p.raw_params)
        hipLaunchKernelGGL(preprocess_geom_kernel<4>, dim3(blocks), dim3(kPreBlock), 0, s, dst, v);
    else
        hipLaunchKernelGGL(preprocess_geom_kernel<0>, dim3(blocks), dim3(kPreBlock), 0, s, dst, v);
}

// ---- the colour sources -----------------------------------------------------------------------------------------------
// Everything that depends on where the colours come from, as data: the three depth-sort launches that carry the source's
// colour role, its stand-alone colour kernel (one argument: the pass block's address -- PreArgs is the block's first
// member, so the kernels that take a PreArgs* get the same value) and the dynamic LDS that role needs.
struct ColorSource {
    void (*sort_step[3])(const FwdPassArgs*, int, int, int);
    const void* color;
    size_t color_lds;
};

static const ColorSource kColorSources[4] = {
    // activated tensors, dense SH [P,M,3]
    {{depth_sort_color_kernel<0, false>, depth_sort_color_kernel<1, false>, depth_sort_color_kernel<2, false>},
     reinterpret_cast<const void*>(preprocess_color_kernel<false, kPreBlock>), kColorLds},
    // activated tensors, ragged degree-sorted SH buffer
    {{depth_sort_color_kernel<0, true>, depth_sort_color_kernel<1, true>, depth_sort_color_kernel<2, true>},
     reinterpret_cast<const void*>(preprocess_color_kernel<true, kPreBlock>), kColorLds},
    // raw parameters: the two SH tensors
    {{depth_sort_color_params_kernel<0>, depth_sort_color_params_kernel<1>, depth_sort_color_params_kernel<2>},
     reinterpret_cast<const void*>(preprocess_color_params_kernel<kPreBlock>), kColorLds},
    // quantised model (kQuantColorLds: 29 KB)
    {{depth_sort_color_quant_kernel<0>, depth_sort_color_quant_kernel<1>, depth_sort_color_quant_kernel<2>},
     reinterpret_cast<const void*>(preprocess_color_quant_kernel<kPreBlock>), kQuantColorLds},
};

static const ColorSource& color_source(const FwdPlan& p)
{
    return kColorSources[p.quant ? 3 : p.raw_params ? 2 : p.ragged ? 1 : 0];
}

void issue_preprocess_color(const FwdPlan& p, const PreArgs* a, hipStream_t s)
{
    const int blocks = pre_chunks(p.P);
    const int grid = p.color_grid > 0 && blocks > p.color_grid ? p.color_grid : blocks;
    const ColorSource& src = color_source(p);
    void* args[] = {&a};
    (void)hipLaunchKernel(src.color, dim3(grid), dim3(kPreBlock), args, src.color_lds, s);
}

static size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

static void opt_in_lds(const void* kernel, size_t bytes)
{
    if (bytes > 48 * 1024) R3_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
}

// Not a stream operation: called before a chain is captured / issued.  hipFuncSetAttribute applies to the CURRENT
// device, so what has been prepared is remembered per device.
void prepare_depth_bucket_sort(int nb)
{
    static std::mutex mu;
    static std::map<int, int> prepared;
    std::lock_guard<std::mutex> lk(mu);
    int dev = 0;
    R3_HIP(hipGetDevice(&dev));
    int& prepared_nb = prepared[dev];
    if (nb <= prepared_nb) return;
    // a launch takes its sort role's size or the colour role's, whichever is larger
    const size_t sort_lds[3] = {depth_hist_lds(nb), depth_scatter_lds(nb), kBucketSortLds};
    for (const ColorSource& src : kColorSources) {
        for (int k = 0; k < 3; k++)
            opt_in_lds(reinterpret_cast<const void*>(src.sort_step[k]), max_sz(sort_lds[k], src.color_lds));
        opt_in_lds(src.color, src.color_lds);
    }
    prepared_nb = nb;
}

// Bucketed depth sort with the SH -> RGB stream riding in spare workgroups of three of its four kernels.  The colour
// chunks are split p.color_split[0..2] percent over the histogram / scatter / bucket-sort launches (each share about
// as long as the sort role it hides behind).
void issue_depth_sort_and_color(const FwdPlan& p, const FwdPassArgs* pa, hipStream_t s)
{
    const int rows = (int)depth_hist_rows((size_t)p.P), nb = p.nb;
    const int chunks = pre_chunks(p.P);
    int c[4] = {0, 0, 0, chunks};
    c[1] = (int)((long long)chunks * p.color_split[0] / 100);
    c[2] = c[1] + (int)((long long)chunks * p.color_split[1] / 100);
    const int cw = p.color_grid > 0 ? p.color_grid : 512;
    const ColorSource& src = color_source(p);
    const int n_sort[3] = {rows, rows, (nb + kBucketsPerGroup - 1) / kBucketsPerGroup};
    const size_t sort_lds[3] = {depth_hist_lds(nb), depth_scatter_lds(nb), kBucketSortLds};
    auto step = [&](int k) {
        const int n_color = c[k + 1] - c[k] < cw ? c[k + 1] - c[k] : cw;
        const size_t lds = n_color ? max_sz(sort_lds[k], src.color_lds) : sort_lds[k];
        hipLaunchKernelGGL(src.sort_step[k], dim3(n_sort[k] + n_color), dim3(kPreBlock), lds, s, pa, n_sort[k], c[k], c[k + 1]);
    };
    step(0);
    hipLaunchKernelGGL(depth_colscan_kernel, dim3((nb + 1 + 63) / 64), dim3(64 * kColWaves), 0, s, &pa->depth);
    step(1);
    step(2);
}

// rasterizer_impl.cu:62-74 checkFrustum: present[i] = (view * p).z > 0.2
__global__ __launch_bounds__(256) void mark_visible_kernel(int P, const float* means, const float* view, bool* present)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    float pv[3];
    xform4x3(view, means[3 * i], means[3 * i + 1], means[3 * i + 2], pv);
    present[i] = pv[2] > 0.2f;
}

void launch_mark_visible(int P, const float* means3D, const float* view, bool* present, hipStream_t s)
{
    hipLaunchKernelGGL(mark_visible_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, means3D, view, present);
}

// r3dgs_activate_params: the activated values the raw-parameter kernels use, by the very functions they call
__global__ __launch_bounds__(256) void activate_params_kernel(int P, const float* __restrict__ scaling_raw,
                                                              const float* __restrict__ rotation_raw,
                                                              float* __restrict__ scales, float* __restrict__ rotations)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    if (scaling_raw && scales)
        for (int k = 0; k < 3; k++) scales[3 * (size_t)i + k] = scale_act(scaling_raw[3 * (size_t)i + k]);
    if (rotation_raw && rotations) {
        const float4 qv = reinterpret_cast<const float4*>(rotation_raw)[i];
        const float rq[4] = {qv.x, qv.y, qv.z, qv.w};
        float q[4];
        quat_act(rq, q);
        reinterpret_cast<float4*>(rotations)[i] = make_float4(q[0], q[1], q[2], q[3]);
    }
}

void launch_activate_params(int P, const float* scaling_raw, const float* rotation_raw, float* scales, float* rotations,
                            hipStream_t s)
{
    hipLaunchKernelGGL(activate_params_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, scaling_raw, rotation_raw, scales,
                       rotations);
}

// r3dgs_quantised_decode: the dense tensors of the reference's load_ply, by the very functions the quantised kernels call
__global__ __launch_bounds__(256) void quantised_decode_kernel(int P, const int* __restrict__ coeffs, const int* __restrict__ perband,
                                                               const int* __restrict__ cumsum, QuantInputs q, float* xyz,
                                                               float* features_dc, float* features_rest, float* opacity,
                                                               float* scaling, float* rotation, int* degrees)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    quant_decode_one(i, coeffs, perband, cumsum, q.xyz, q.xyz_is_half, q.geom_ids, q.sh_ids, q.codebooks, xyz, features_dc,
                     features_rest, opacity, scaling, rotation, degrees);
}

void launch_quantised_decode(int P, const int* coeffs, const int* perband, const int* cumsum, const QuantInputs& q, float* xyz,
                             float* features_dc, float* features_rest, float* opacity, float* scaling, float* rotation,
                             int* degrees, hipStream_t s)
{
    hipLaunchKernelGGL(quantised_decode_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, coeffs, perband, cumsum, q, xyz,
                       features_dc, features_rest, opacity, scaling, rotation, degrees);
}

}  // namespace r3
