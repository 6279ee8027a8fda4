// blend.hip -- per-tile front-to-back alpha blending (forward) and its per-pixel backward, gfx950.
//
// Replaces cuda_rasterizer/forward.cu:461-582 renderCUDA and backward.cu:437-595 renderCUDA of
// /root/reference/submodules/diff-gaussian-rasterization.
//
// MI355X-first structure (not the reference's 256-thread block with two barriers per chunk):
//   * ONE 64-lane wave owns a pixel region of a tile and streams the tile's list on its own: single-wave
//     workgroups, no cross-wave barriers, so the CU's wave slots hide each other's gather latency.  A lane
//     carries PPL pixels (PPL 8x8 quadrants of the 16x16 tile): every LDS broadcast read of a Gaussian record
//     is amortised over PPL pixels per lane, and the backward's cross-lane reduction over PPL x 64 pixels.
//   * the list is fetched 64 entries at a time: lane j gathers the 48-byte GRec of entry j (one
//     cache-line-local load instead of the reference's five scattered arrays) into registers one chunk
//     ahead of its use, then parks it in LDS.
//   * while it holds entry j, lane j also runs the exact region pre-test (blend_math.h): more than half of
//     the reference's bounding-square tile entries reach no pixel of the tile, 72% no pixel of a given
//     quadrant.  The wave then walks only the surviving entries (bit scan over a wave-uniform mask) and
//     only their surviving quadrants.  Per-pixel decisions are untouched, so image, n_contrib and gradients
//     are what they are without the pre-test.
//   * the forward keeps its pre-test masks (one 64-bit word per chunk and quadrant) and the backward loads them
//     instead of repeating the minimisation.
//   * the conic is pre-scaled when an entry is staged, so that log2(G) is three FMAs per (pixel, entry); the
//     backward accumulates moments of m = G * dL/dalpha (sum m, sum m d, sum m d d^T) per pixel and forms the
//     gradients once per (tile, entry).
//   * backward: the 9 sums of an entry are added over the lane's pixels, reduced across the wave with DPP row
//     operations (bank-masked adds, wave_reduce9 below; finishing the last steps with 4 same-address LDS float
//     atomics instead was measured 45% slower), parked in LDS per list entry, and flushed once per 64-entry chunk
//     with plain stores into the entry's own slot of a per-(tile, Gaussian)-pair slab.  The reference issues
//     one global float atomic per (pixel, Gaussian, component); a first version here issued one per (tile,
//     Gaussian, component) and still spent 0.25 of 0.87 ms on them (11.8 M atomics per pass at the BASELINE
//     shape).  Now there are none: the per-Gaussian kernel sums a Gaussian's slots, which are contiguous.
//   * workgroup ids are remapped so that consecutive tiles run on the same XCD (shared L2 for the records of
//     Gaussians straddling neighbouring tiles).
#include <cstdlib>

#include "blend_math.h"
#include "common.h"
#include "unit_order.h"

namespace r3 {

// (pointers out of a pass block go through global_ptr(), common.h: FLAT accesses would count on lgkmcnt and every wait for an
// LDS read would wait for the global gather in flight)
constexpr int kChunk = 64;

// debug builds only (tools/bwd_timeline.py): when and where every workgroup of the backward (-DR3_TIMELINE) or of the
// forward (-DR3_TIMELINE_FWD) blend ran
#if defined(R3_TIMELINE) || defined(R3_TIMELINE_FWD)
__device__ unsigned long long g_timeline[4 * 65536];
#define R3_TL_BEGIN_(id) const unsigned long long tl0_ = __builtin_amdgcn_s_memtime(); const uint32_t tlid_ = (id);
#define R3_TL_END_(extra)                                                                                                \
    if (threadIdx.x == 0 && tlid_ < 65536u) {                                                                            \
        g_timeline[4 * tlid_] = tl0_;                                                                                     \
        g_timeline[4 * tlid_ + 1] = __builtin_amdgcn_s_memtime();                                                         \
        g_timeline[4 * tlid_ + 2] = (unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)) |     \
                                    ((unsigned long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)) << 32); \
        g_timeline[4 * tlid_ + 3] = (unsigned long long)(extra);                                                          \
    }
#endif
#if defined(R3_TIMELINE)
#define R3_TL_BEGIN(id) R3_TL_BEGIN_(id)
#define R3_TL_END(extra) R3_TL_END_(extra)
#else
#define R3_TL_BEGIN(id)
#define R3_TL_END(extra)
#endif
#if defined(R3_TIMELINE_FWD)
#define R3_TLF_BEGIN(id) R3_TL_BEGIN_(id)
#define R3_TLF_END(extra) R3_TL_END_(extra)
#else
#define R3_TLF_BEGIN(id)
#define R3_TLF_END(extra)
#endif

struct LdsRec {  // 48 B: a staged list entry, conic pre-scaled (QSplat); c.yzw = GRec's rect_min, width_clamp, pair_start
    float4 a;    // x, y, qa, qb
    float4 b;    // qc, op, r, g
    float4 c;    // b, -, -, -
};

__device__ __forceinline__ QSplat load_splat(const LdsRec& r)
{
    QSplat s;
    s.x = r.a.x;
    s.y = r.a.y;
    s.qa = r.a.z;
    s.qb = r.a.w;
    s.qc = r.b.x;
    s.op = r.b.y;
    s.r = r.b.z;
    s.g = r.b.w;
    s.b = r.c.x;
    return s;
}

__device__ __forceinline__ Splat splat_from_regs(const float4& a, const float4& b, const float4& c)
{
    Splat s;
    s.x = a.x;
    s.y = a.y;
    s.cA = a.z;
    s.cB = a.w;
    s.cC = b.x;
    s.op = b.y;
    s.r = b.z;
    s.g = b.w;
    s.b = c.x;
    return s;
}

// Lane j parks the entry it gathered (registers a, b, c = the GRec) with the conic pre-scaled.  Six narrow stores, each
// either straight out of the gather's destination registers or of freshly computed values: built as three float4
// the compiler shuffles the loaded components into new register tuples right behind the gather -- and waits for the
// gather there, which serialises the prefetch of chunk k+1 with the blending of chunk k.
__device__ __forceinline__ void stage_entry(LdsRec& dst, const float4& a, const float4& b, const float4& c)
{
    typedef float v2f __attribute__((ext_vector_type(2)));
    typedef float v4f __attribute__((ext_vector_type(4)));
    // volatile: or the stores are merged back into float4; explicitly LDS: volatile accesses are not address-space inferred
#define R3_LDS_V(T) volatile T __attribute__((address_space(3)))*
    R3_LDS_V(float) d = (R3_LDS_V(float))reinterpret_cast<float*>(&dst);
    *(R3_LDS_V(v2f))d = v2f{a.x, a.y};
    *(R3_LDS_V(v2f))(d + 2) = v2f{(-0.5f * kLog2e) * a.z, -kLog2e * a.w};
    d[4] = (-0.5f * kLog2e) * b.x;
    d[5] = b.y;
    *(R3_LDS_V(v2f))(d + 6) = v2f{b.z, b.w};
    *(R3_LDS_V(v4f))(d + 8) = v4f{c.x, c.y, c.z, c.w};
#undef R3_LDS_V
}

// The forward does not need c.yzw; it parks the entry's 1-based list position in c.y instead, so that the position comes
// back with the record's last word (one ds_read_b64) as a VGPR: n_contrib = pos is then a full-rate v_mov from a VGPR instead
// of an s_add + v_mov from an SGPR (half rate), paid once per chunk and lane here instead of once per blended entry.
__device__ __forceinline__ void stage_entry_fwd(LdsRec& dst, const float4& a, const float4& b, const float4& c, uint32_t pos1)
{
    typedef float v2f __attribute__((ext_vector_type(2)));
#define R3_LDS_V(T) volatile T __attribute__((address_space(3)))*
    R3_LDS_V(float) d = (R3_LDS_V(float))reinterpret_cast<float*>(&dst);
    *(R3_LDS_V(v2f))d = v2f{a.x, a.y};
    *(R3_LDS_V(v2f))(d + 2) = v2f{(-0.5f * kLog2e) * a.z, -kLog2e * a.w};
    d[4] = (-0.5f * kLog2e) * b.x;
    d[5] = b.y;
    *(R3_LDS_V(v2f))(d + 6) = v2f{b.z, b.w};
    d[8] = c.x;
    d[9] = __uint_as_float(pos1);
#undef R3_LDS_V
}

__device__ __forceinline__ uint32_t staged_pos1(const LdsRec& r) { return __float_as_uint(r.c.y); }

// consecutive logical ids on one XCD: hardware places workgroup b on XCD b % 8 (speed only, never correctness)
__device__ __forceinline__ uint32_t xcd_remap(uint32_t b, uint32_t nblocks)
{
    const uint32_t per = nblocks >> 3;
    if (b >= per * 8) return b;  // tail
    return (b & 7u) * per + (b >> 3);
}

// mask &= ~(1 << j) on the scalar unit in ONE instruction (the compiler's  m & (m - 1)  is s_add_u32 + s_addc_u32 + s_and_b64;
// the scalar unit of a CU is shared by its four SIMDs and more than half busy in the forward)
__device__ __forceinline__ void clear_bit(unsigned long long& mask, int j)
{
#ifdef R3_OLD_TRIP_FORMS
    mask &= ~(1ull << j);
#else
    asm("s_bitset0_b64 %0, %1" : "+s"(mask) : "s"(j));
#endif
}

#define R3_DPP_ADD(v, ctrl, rmask) \
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, rmask, 0xf, true))

// sum over each 16-lane DPP row, result in every lane of the row
__device__ __forceinline__ float row_sum(float v)
{
    R3_DPP_ADD(v, 0xb1, 0xf);   // quad_perm [1,0,3,2]
    R3_DPP_ADD(v, 0x4e, 0xf);   // quad_perm [2,3,0,1]
    R3_DPP_ADD(v, 0x124, 0xf);  // row_ror:4
    R3_DPP_ADD(v, 0x128, 0xf);  // row_ror:8
    return v;
}

// full-wave sum; result valid in lane 63
__device__ __forceinline__ float wave_sum_to_lane63(float v)
{
    v = row_sum(v);
    R3_DPP_ADD(v, 0x142, 0xa);  // row_bcast:15 into rows 1 and 3
    R3_DPP_ADD(v, 0x143, 0xc);  // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave sum
    return v;
}

// Transposing wave reduction of the 9 per-entry sums (SplatSums, in its field order: components 0..8).  A plain butterfly
// costs 6 cross-lane adds per component (54, and the two cross-row steps need an extra move each).  Here every step
// over a lane bit exchanges DIFFERENT components between partner lanes (keep one, send the other), halving the live
// registers: 9 -> 5 -> 3 -> 2 -> 1, and only that one register crosses the 16-lane rows (2 ds_bpermute).  The two
// steps that start with the most registers go over lane bits 2 and 3 (row_ror:4 / row_ror:8), because a DPP bank mask
// selects exactly those bits (bank = 4 consecutive lanes of a row): two bank-masked v_add_f32_dpp into the same
// destination do "keep mine, add the partner's" without a v_cndmask.  The compiler cannot be asked for a bank-masked
// DPP add (it only folds full-mask moves), so those 14 instructions are inline assembly; the leading s_nop is the
// VALU-write -> DPP-read wait states the hazard recogniser cannot see INTO an asm block (it does pad behind one).
// Afterwards every lane with (lane & 2) == 0 holds the wave total of component reduce9_component(lane), every other
// lane component 8.  25 VALU + 2 DS per entry (was 38 + 6).
__device__ __forceinline__ int reduce9_component(int lane)
{
    return (lane & 2) ? 8 : 4 * (lane & 1) + 2 * ((lane >> 3) & 1) + ((lane >> 2) & 1);
}

__device__ __forceinline__ float wave_reduce9(const SplatSums& g, int lane)
{
    float u0, u1, u2, u3, t8, w0, w1;
    asm("s_nop 1\n\t"
        // lane bit 2: banks 0 and 2 keep the first of a pair, banks 1 and 3 the second
        "v_add_f32_dpp %[u0], %[mx], %[mx] row_ror:4 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %[u0], %[my], %[my] row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %[u1], %[ca], %[ca] row_ror:4 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %[u1], %[cb], %[cb] row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %[u2], %[cc], %[cc] row_ror:4 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %[u2], %[op], %[op] row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %[u3], %[cr], %[cr] row_ror:4 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %[u3], %[cg], %[cg] row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %[t8], %[bl], %[bl] row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
        // lane bit 3: banks 0 and 1 keep the first, banks 2 and 3 the second
        "v_add_f32_dpp %[w0], %[u0], %[u0] row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %[w0], %[u1], %[u1] row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %[w1], %[u2], %[u2] row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %[w1], %[u3], %[u3] row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %[t8], %[t8], %[t8] row_ror:8 row_mask:0xf bank_mask:0xf"
        : [u0] "=&v"(u0), [u1] "=&v"(u1), [u2] "=&v"(u2), [u3] "=&v"(u3), [t8] "=&v"(t8), [w0] "=&v"(w0), [w1] "=&v"(w1)
        : [mx] "v"(g.sx), [my] "v"(g.sy), [ca] "v"(g.sxx), [cb] "v"(g.sxy), [cc] "v"(g.syy), [op] "v"(g.sm), [cr] "v"(g.r),
          [cg] "v"(g.g), [bl] "v"(g.b));
    // now, summed over the 4 lanes of the row with the same lane & 3:  w0 = component 2 * bit3 + bit2,  w1 = 4 + that,  t8 = b
    R3_DPP_ADD(w0, 0xb1, 0xf);   // quad_perm [1,0,3,2]
    R3_DPP_ADD(w1, 0xb1, 0xf);
    R3_DPP_ADD(t8, 0xb1, 0xf);
    float z = (lane & 1) ? w1 : w0;
    R3_DPP_ADD(z, 0x4e, 0xf);    // quad_perm [2,3,0,1]
    R3_DPP_ADD(t8, 0x4e, 0xf);
    z = (lane & 2) ? t8 : z;
    z += __shfl_xor(z, 16);
    z += __shfl_xor(z, 32);
    return z;
}

// The two abs sums of an ABS pass (blend_math.h SplatAbsSums), reduced the same transposing way: the first step exchanges
// the two between partner lanes, one register goes through the other five.  Afterwards every even lane holds the wave total
// of ax and every odd lane that of ay.  7 VALU + 2 DS per reduced entry.
__device__ __forceinline__ float wave_reduce2(float ax, float ay, int lane)
{
    R3_DPP_ADD(ax, 0xb1, 0xf);   // quad_perm [1,0,3,2]
    R3_DPP_ADD(ay, 0xb1, 0xf);
    float z = (lane & 1) ? ay : ax;
    R3_DPP_ADD(z, 0x4e, 0xf);    // quad_perm [2,3,0,1]
    R3_DPP_ADD(z, 0x124, 0xf);   // row_ror:4
    R3_DPP_ADD(z, 0x128, 0xf);   // row_ror:8
    z += __shfl_xor(z, 16);
    z += __shfl_xor(z, 32);
    return z;
}

template <int PPL>
__device__ __forceinline__ void pixel_of(int tile_x, int tile_y, int part, int q, int lane, int* px, int* py)
{
    const int b4 = part * PPL + q;  // 8x8 quadrant inside the 16x16 tile
    *px = tile_x * kTile + (b4 & 1) * 8 + (lane & 7);
    *py = tile_y * kTile + (b4 >> 1) * 8 + (lane >> 3);
}

constexpr int kFwdBatch = 4;   // entries per trip of the forward's entry loop: 2 / 3 / 4 -> 0.163 / 0.158 / 0.158 ms

// Blends batches of N surviving entries (front to back) while at least N survive; returns the entries left over.
template <int N, int PPL>
__device__ __forceinline__ unsigned long long fwd_batches(unsigned long long anymask, const unsigned long long* qmask,
                                                          const LdsRec* s_rec, const float* pxf, const float* pyf,
                                                          FwdPix* pix)
{
    // the survivors are counted once and the count carried in a scalar register: `popcount(mask) >= N` per trip is an
    // s_bcnt1 and a 64-bit VECTOR compare (there is no scalar one for "greater")
    for (int left = __builtin_popcountll(anymask); left >= N; left -= N) {
        int j[N];
        QSplat sp[N];
        uint32_t pos1[N];
        float al[N][PPL];
        bool inb[N][PPL];
#pragma unroll
        for (int i = 0; i < N; i++) {
            j[i] = __builtin_ctzll(anymask);
            clear_bit(anymask, j[i]);
            sp[i] = load_splat(s_rec[j[i]]);
            pos1[i] = staged_pos1(s_rec[j[i]]);
        }
#pragma unroll
        for (int i = 0; i < N; i++)
#pragma unroll
            for (int q = 0; q < PPL; q++) al[i][q] = fwd_alpha(sp[i], pxf[q], pyf[q], &inb[i][q]);
#pragma unroll
        for (int i = 0; i < N; i++)
#pragma unroll
            for (int q = 0; q < PPL; q++)
                if (PPL == 1 || ((qmask[q] >> j[i]) & 1ull)) {   // one quadrant per wave: anymask IS its mask
                    float Tb;
                    fwd_apply(sp[i], al[i][q], inb[i][q], pos1[i], pix[q], &Tb);
                }
    }
    return anymask;
}

template <int PPL, bool COUNTERS>
__global__ __launch_bounds__(64) void blend_fwd_kernel(const BlendFwdArgs* __restrict__ ap)
{
    __shared__ LdsRec s_rec[kChunk];
    const BlendFwdArgs a = *ap;   // pass block in device memory: scalar loads, once
    R3_TLF_BEGIN(blockIdx.x)
    __shared__ uint32_t s_id[kChunk];
    constexpr int PARTS = 4 / PPL;
    const int lane = threadIdx.x;
    const uint32_t wg = xcd_remap(blockIdx.x, a.nblocks);
    const uint32_t tile = wg / PARTS;
    const int part = (int)(wg % PARTS);
    const int tile_x = (int)(tile % (uint32_t)a.gx), tile_y = (int)(tile / (uint32_t)a.gx);
    // (stays in VGPRs: made wave-uniform by readfirstlane, the scalar loop control cost 0.174 -> 0.185 ms here)
    const uint2 range = global_ptr(a.ranges)[tile];

    float pxf[PPL], pyf[PPL], qx0[PPL], qy0[PPL];
    FwdPix pix[PPL];
    bool inside[PPL];
#pragma unroll
    for (int q = 0; q < PPL; q++) {
        int px, py;
        pixel_of<PPL>(tile_x, tile_y, part, q, lane, &px, &py);
        const int b4 = part * PPL + q;
        qx0[q] = (float)(tile_x * kTile + (b4 & 1) * 8);   // first pixel column / row of quadrant q: wave-uniform,
        qy0[q] = (float)(tile_y * kTile + (b4 >> 1) * 8);  // computed from scalars so that it stays in SGPRs
        pxf[q] = (float)px;
        pyf[q] = (float)py;
        inside[q] = px < a.W && py < a.H;
        fwd_pix_init(pix[q], inside[q]);
    }

    // software pipeline: the records of chunk k+1 are gathered into registers while chunk k is blended
    // A list this long may be walked in segments by the backward (common.h): the state in front of every S-th entry is
    // parked for it while the walk is here anyway (4 KB per tile and checkpoint; nothing for the other tiles)
    const uint32_t seg_log2 = a.ckpt ? global_ptr(a.hdr)->ckpt : 0u;
    const bool segmented = seg_log2 != 0u && range.y - range.x >= global_ptr(a.hdr)->ckpt_thr;
    float4 nxa, nxb, nxc;
    uint32_t nxid = 0;
    nxa = nxb = nxc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (range.x + lane < range.y) {
        nxid = global_ptr(a.point_list)[range.x + lane];
        const auto* g = (const R3_GLOBAL float4*)global_ptr(a.rec + nxid);
        nxa = g[0];
        nxb = g[1];
        nxc = g[2];
    }
    // the list ids run one more chunk ahead than the records they index: one memory round trip per chunk, not two
    uint32_t nnid = 0;
    if (range.x + kChunk + lane < range.y) nnid = global_ptr(a.point_list)[range.x + kChunk + lane];
    for (uint32_t base = range.x; base < range.y; base += kChunk) {
        {
            bool live = false;
#pragma unroll
            for (int q = 0; q < PPL; q++) live |= fwd_pix_live(pix[q]);
            if (__ballot(live) == 0ull) break;  // every pixel of the region saturated
        }
        if (segmented) {
            const uint32_t rel = base - range.x;
            if (rel != 0u && (rel & ((1u << seg_log2) - 1u)) == 0u && (rel >> seg_log2) < (uint32_t)kFwdCkptMax) {
                auto* dst = global_ptr(a.ckpt) + ckpt_slot(range.x, rel >> seg_log2, tile, seg_log2) * 256;
#pragma unroll
                for (int q = 0; q < PPL; q++)   // a pixel that is done by now is never looked up here
                    dst[(part * PPL + q) * 64 + lane] = make_float4(pix[q].T, pix[q].C0, pix[q].C1, pix[q].C2);
            }
        }
        __syncthreads();
        stage_entry_fwd(s_rec[lane], nxa, nxb, nxc, base - range.x + (uint32_t)lane + 1u);
        if (COUNTERS) s_id[lane] = nxid;
        // region pre-test: lane j decides for entry j which of this wave's quadrants it can reach at all
        unsigned long long qmask[PPL], anymask = 0ull;
        {
            const Splat mine = splat_from_regs(nxa, nxb, nxc);
            const bool have = base + lane < range.y;
#pragma unroll
            for (int q = 0; q < PPL; q++) {
                qmask[q] = __ballot(have && region_may_contribute(mine, qx0[q], qx0[q] + 7.f, qy0[q], qy0[q] + 7.f));
                anymask |= qmask[q];
            }
            if (a.quad_masks) {   // kept for the backward, which walks the same chunks
                auto* dst =
                    global_ptr(a.quad_masks) + quad_mask_slot(range.x, (base - range.x) >> 6, tile) * 4 + (uint32_t)(part * PPL);
                if (lane == 0) {
#pragma unroll
                    for (int q = 0; q < PPL; q++) dst[q] = qmask[q];
                }
            }
        }
        __syncthreads();
        {
            const uint32_t idx = base + kChunk + lane;
            if (idx < range.y) {
                nxid = nnid;
                const auto* g = (const R3_GLOBAL float4*)global_ptr(a.rec + nxid);
                nxa = g[0];
                nxb = g[1];
                nxc = g[2];
            }
            if (idx + kChunk < range.y) nnid = global_ptr(a.point_list)[idx + kChunk];
        }
        // Several surviving entries per trip: their alphas (the exp and the quadratic form, ~70 % of a step) do not depend on
        // the pixel state, so they are evaluated side by side before the sequential compositing of one after the other
        // -- independent work between dependent instructions, and the scalar loop control (bit scan, LDS address, branch)
        // is paid once per batch: the forward is as sensitive to those as to vector instructions (one entry per trip 0.176 ms,
        // two 0.171, two without per-entry "is there a second one" tests 0.159, four 0.158).
        if (!COUNTERS) {
            anymask = fwd_batches<kFwdBatch, PPL>(anymask, qmask, s_rec, pxf, pyf, pix);
            anymask = fwd_batches<2, PPL>(anymask, qmask, s_rec, pxf, pyf, pix);
        }
        while (anymask) {  // surviving entries, front to back
            const int j = __builtin_ctzll(anymask);
            clear_bit(anymask, j);
            const QSplat s = load_splat(s_rec[j]);
            const uint32_t pos1 = staged_pos1(s_rec[j]);
            int cnt = 0;
            float tsum = 0.f;
#pragma unroll
            for (int q = 0; q < PPL; q++) {
                if ((qmask[q] >> j) & 1ull) {
                    float Tb;
                    const int r = fwd_step(s, pxf[q], pyf[q], pos1, pix[q], &Tb);
                    if (COUNTERS && r == 1) {
                        cnt++;
                        tsum += Tb;
                    }
                }
            }
            if (COUNTERS) {  // forward.cu:560-564, one atomic pair per (region, Gaussian) instead of per pixel
                if (__ballot(cnt != 0) != 0ull) {
                    const float c = wave_sum_to_lane63((float)cnt);
                    const float t = wave_sum_to_lane63(tsum);
                    if (lane == 63) {
                        atomicAdd(a.touched + s_id[j], (int)c);
                        atomicAdd(a.transmittance + s_id[j], t);
                    }
                }
            }
        }
    }
    // deepest contributor of each quadrant: how far the backward will have to walk this tile's list (its launch order)
#pragma unroll
    for (int q = 0; q < PPL; q++) {
        uint32_t m = pix[q].last;
        for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
        if (lane == 0) global_ptr(a.quad_depth)[tile * 4u + (uint32_t)(part * PPL + q)] = m;
    }
    if (segmented) {   // slot 0: the colour every contributor left (without the background): what lies behind a checkpoint
        auto* dst = global_ptr(a.ckpt) + ckpt_slot(range.x, 0u, tile, seg_log2) * 256;
#pragma unroll
        for (int q = 0; q < PPL; q++)
            dst[(part * PPL + q) * 64 + lane] = make_float4(fwd_pix_T(pix[q]), pix[q].C0, pix[q].C1, pix[q].C2);
    }
    const size_t plane = (size_t)a.W * a.H;
    const float bg0 = global_ptr(a.bg)[0], bg1 = global_ptr(a.bg)[1], bg2 = global_ptr(a.bg)[2];
#pragma unroll
    for (int q = 0; q < PPL; q++) {
        if (inside[q]) {
            const size_t p = (size_t)a.W * (size_t)pyf[q] + (size_t)pxf[q];
            const float T = fwd_pix_T(pix[q]);
            global_ptr(a.final_T)[p] = T;
            global_ptr(a.n_contrib)[p] = pix[q].last;
            global_ptr(a.out_color)[p] = pix[q].C0 + T * bg0;
            global_ptr(a.out_color)[plane + p] = pix[q].C1 + T * bg1;
            global_ptr(a.out_color)[2 * plane + p] = pix[q].C2 + T * bg2;
        }
    }
    R3_TLF_END(range.y - range.x)
}

// One pixel per lane, four workgroups per tile: 2 / 4 pixels per lane measured 0.188 / 0.225 against 0.179 ms.
void issue_blend_forward(const FwdPlan& p, const BlendFwdArgs* a, hipStream_t s)
{
    const uint32_t nblocks = (uint32_t)(p.gx * p.gy * 4);   // == a->nblocks
    if (p.counters)
        hipLaunchKernelGGL((blend_fwd_kernel<1, true>), dim3(nblocks), dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL((blend_fwd_kernel<1, false>), dim3(nblocks), dim3(64), 0, s, a);
}

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
constexpr int kGradStride = 9;   // the 9 sums of a list entry (odd stride: the flush reads without bank conflicts)
constexpr int kGradStrideAbs = 11;   // ABS: and the two abs sums (still odd)

// REUSE: the region pre-test masks are the forward's (BinState::quad_masks) instead of being recomputed per chunk.
// 6 waves per SIMD (80 VGPRs, three spilled values outside the entry loop).  With round 2's 96-register body 5 and 6
// measured the same; since the accumulated-colour recurrence and the offset products took 10 registers out of the
// loop, 6 is the faster by 1 % (0.3602 / 0.3603 vs 0.3644 / 0.3627 ms, two runs each, same box).
// One workgroup = one UNIT: a tile, or -- for a tile whose list the pass splits (common.h) -- entries [lo, hi) of
// its list.  A segment that ends in front of a pixel's last contributor starts that pixel from the forward's checkpoint at
// `hi`: T there, and the colour that lies behind it = (final colour - colour in front of hi) / T, projected on the pixel's
// upstream gradient (the accumulated-colour state A of blend_math.h BwdPix); a pixel whose last contributor is inside
// [lo, hi) starts as ever, one that ends in front of lo has nothing to do here.  Every list entry belongs to exactly one
// segment, so every row of the per-pair slab still has ONE writer: no atomics, bit-reproducible.
// FIRST: this is the first kernel of the backward (no unit order): it installs the pass block for the kernels behind it and
// reads its own arguments from the kernarg segment; otherwise unit_order_kernel (unit_order.hip) did and the arguments come from the block
// (a graph replay refreshes the by-value arguments of its first node only).
// ABS (r3dgs_backward_absgrad): the walk also sums, per entry, the absolute values of what each pixel adds to dL_dmean2D
// (blend_math.h bwd_accumulate_abs): 11 sums per entry are accumulated, reduced, parked and cleared, and the two abs columns
// leave in columns 9 and 10 of the entry's slab row, which the other instantiations write as zeros.  Its register budget is
// its own (bwd_waves below); the instantiations without ABS are compiled exactly as before the parameter existed.
// Waves per SIMD: 6 as ever without ABS.  With ABS the body needs 93 VGPRs (REUSE) / 98 (the pre-test repeated): 5 waves hold
// the first without a spill and the second only with one, so that one is built for 4 (rule 1: a wave is
// not bought with spills; profiles/absgrad_kernel_resources.txt).
constexpr int bwd_waves(bool reuse, bool abs) { return abs ? (reuse ? 5 : 4) : 6; }
template <int PPL, bool REUSE, bool FIRST, bool ABS = false>
__global__ __launch_bounds__(64, bwd_waves(REUSE, ABS)) void blend_bwd_kernel(BwdPassArgs* dst, BwdPassArgs v)
{
    constexpr int GS = ABS ? kGradStrideAbs : kGradStride;
    __shared__ LdsRec s_rec[kChunk];
    if (FIRST && blockIdx.x == 0) install_block_from_kernarg(dst, (int)threadIdx.x, 64);
    R3_TL_BEGIN(blockIdx.x)
    const BlendBwdArgs a = FIRST ? v.blend : dst->blend;
    __shared__ float s_grad[kChunk * GS];
#ifndef R3_OLD_TRIP_FORMS
    __shared__ float4 s_zero[3];   // nine zeros (and three spare): what the sums of an entry are reset from, see below
    if (threadIdx.x < 3) s_zero[threadIdx.x] = make_float4(0.f, 0.f, 0.f, 0.f);
#endif
    constexpr int PARTS = 4 / PPL;
    const int lane = threadIdx.x;
    uint32_t wg, seg = 0u, nseg = 1u, walk_log2 = 0u;
    if (a.unit_order) {
        // entry b / lists of list b % lists (each list is heaviest first; the grid covers the most units a pass may have)
        const uint32_t g = blockIdx.x % kOrderLists, i = blockIdx.x / kOrderLists;
        const uint32_t* trailer = unit_trailer_at(a.unit_order, a.units_cap, g);
        if (i >= trailer[0]) return;
        walk_log2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)trailer[1]);   // segment length this list's units walk
        const Unit u = unit_unpack(
            (uint32_t)__builtin_amdgcn_readfirstlane((int)a.unit_order[unit_list_base(a.units_cap, g) + i]));
        wg = u.tile;
        seg = u.segment;
        nseg = u.segments;
    } else {
        wg = xcd_remap(blockIdx.x, a.nblocks);
    }
    const uint32_t tile = wg / PARTS;
    const int part = (int)(wg % PARTS);
    const int tile_x = (int)(tile % (uint32_t)a.gx), tile_y = (int)(tile / (uint32_t)a.gx);
    uint2 range = a.ranges[tile];
    range.x = (uint32_t)__builtin_amdgcn_readfirstlane((int)range.x);   // wave-uniform: kept in SGPRs
    range.y = (uint32_t)__builtin_amdgcn_readfirstlane((int)range.y);
    const size_t plane = (size_t)a.W * a.H;
    const float bg0 = a.bg[0], bg1 = a.bg[1], bg2 = a.bg[2];

    float pxf[PPL], pyf[PPL], qx0[PPL], qy0[PPL];
    BwdPix pix[PPL];
    uint32_t lmax = 0;
#pragma unroll
    for (int q = 0; q < PPL; q++) {
        int px, py;
        pixel_of<PPL>(tile_x, tile_y, part, q, lane, &px, &py);
        const int b4 = part * PPL + q;
        qx0[q] = (float)(tile_x * kTile + (b4 & 1) * 8);
        qy0[q] = (float)(tile_y * kTile + (b4 >> 1) * 8);
        pxf[q] = (float)px;
        pyf[q] = (float)py;
        const bool inside = px < a.W && py < a.H;
        BwdPix& p = pix[q];
        bwd_pix_init(p, 0.f, 0u, 0.f, 0.f, 0.f, 0.f);
        if (inside) {
            const size_t id = (size_t)a.W * py + px;
            const float g0 = a.dL_dpix[id], g1 = a.dL_dpix[plane + id], g2 = a.dL_dpix[2 * plane + id];
            bwd_pix_init(p, a.final_T[id], a.n_contrib[id], g0, g1, g2, bg0 * g0 + bg1 * g1 + bg2 * g2);
        }
        lmax = max(lmax, p.last);
    }
    // deepest contributor of each quadrant and of the whole region: nothing behind it matters to any pixel there
    uint32_t qlast[PPL];
#pragma unroll
    for (int q = 0; q < PPL; q++) {
        uint32_t m = pix[q].last;
        for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
        qlast[q] = (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
    }
    for (int off = 32; off > 0; off >>= 1) lmax = max(lmax, (uint32_t)__shfl_xor((int)lmax, off));
    lmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)lmax);
    if (lmax == 0) {
        R3_TL_END(0)
        return;
    }
    // this unit's part of the list: [lo, hi)
    uint32_t lo = 0u, hi = lmax;
    if (nseg > 1u) {
        lo = seg << walk_log2;
        if (seg + 1u < nseg) hi = lo + (1u << walk_log2);   // (the unit order only makes segments with lo < lmax)
        if (hi < lmax) {
            // pixels whose last contributor lies behind this segment pass through it: their state in front of entry `hi`
            // (the forward's checkpoints are S = 2^hdr->ckpt apart; a pass may walk segments of 2 S, 4 S ...)
            const uint32_t seg_log2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.hdr->ckpt);
            const float4* ck = a.ckpt + ckpt_slot(range.x, hi >> seg_log2, tile, seg_log2) * 256;
            const float4* fin = a.ckpt + ckpt_slot(range.x, 0u, tile, seg_log2) * 256;
#pragma unroll
            for (int q = 0; q < PPL; q++) {
                BwdPix& p = pix[q];
                if (p.last > hi) {
                    const float4 c = ck[(part * PPL + q) * 64 + lane], f = fin[(part * PPL + q) * 64 + lane];
                    // p.T is the final transmittance here and p.A the background term bg . g
                    p.A = ((f.y - c.y) * p.g0 + (f.z - c.z) * p.g1 + (f.w - c.w) * p.g2 + p.T * p.A) * R3_RCP(c.x);
                    p.T = c.x;
                }
            }
#pragma unroll
            for (int q = 0; q < PPL; q++) qlast[q] = min(qlast[q], hi);
        }
    }

    const float half_w = 0.5f * (float)a.W, half_h = 0.5f * (float)a.H;  // backward.cu:498-499
    float4 nxa, nxb, nxc;
    uint32_t nxid = 0;
    nxa = nxb = nxc = make_float4(0.f, 0.f, 0.f, 0.f);
    const int cfirst = (int)((hi - 1) / kChunk) * kChunk;
    if ((uint32_t)cfirst + (uint32_t)lane < hi) {
        nxid = a.point_list[range.x + (uint32_t)cfirst + (uint32_t)lane];
        const float4* g = reinterpret_cast<const float4*>(a.rec + nxid);
        nxa = g[0];
        nxb = g[1];
        nxc = g[2];
    }
    uint32_t nnid = 0;   // list ids run one more chunk ahead than the records they index
    if (cfirst >= kChunk) nnid = a.point_list[range.x + (uint32_t)(cfirst - kChunk) + (uint32_t)lane];
    // the forward's masks of a chunk travel with its records: lane q < 4 fetches quadrant q's word one chunk ahead
    const unsigned long long* const masks0 = REUSE ? a.quad_masks + quad_mask_slot(range.x, 0u, tile) * 4 : nullptr;
    unsigned long long nxm = 0ull;
    if (REUSE && lane < 4) nxm = masks0[(size_t)(cfirst >> 6) * 4 + lane];
    // lanes that park the reduced sums of an entry: lane -> component as wave_reduce9 leaves them
    const bool writer = lane < 16 && ((lane & 2) == 0 || lane == 2);
    float* const s_grad_slot = s_grad + reduce9_component(lane);
    SplatSums sg;   // zero whenever an entry starts: cleared after every reduction, untouched by entries without a hit
    sg.sx = sg.sy = sg.sxx = sg.sxy = sg.syy = sg.sm = sg.r = sg.g = sg.b = 0.f;
    SplatAbsSums sa;   // ABS only
    sa.ax = sa.ay = 0.f;
    for (int cbase = cfirst; cbase >= (int)lo; cbase -= kChunk) {
        __syncthreads();
        stage_entry(s_rec[lane], nxa, nxb, nxc);
        unsigned long long qmask[PPL], anymask = 0ull;
        {
            const Splat mine = splat_from_regs(nxa, nxb, nxc);
            const bool have = (uint32_t)cbase + (uint32_t)lane < hi;
#pragma unroll
            for (int q = 0; q < PPL; q++) {
                if (REUSE) {
                    const uint32_t mlo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)nxm, q);
                    const uint32_t mhi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(nxm >> 32), q);
                    qmask[q] = ((unsigned long long)mhi << 32) | mlo;
                } else {
                    qmask[q] = __ballot(have && region_may_contribute(mine, qx0[q], qx0[q] + 7.f, qy0[q], qy0[q] + 7.f));
                }
                // entries behind the quadrant's deepest contributor / behind this unit's segment (scalar arithmetic)
                // (signed: written as an unsigned saturating difference this has no scalar instruction and came out as
                // v_mov + v_sub clamp + v_cmp + v_readfirstlane per quadrant and chunk)
                const int left = max((int)qlast[q] - cbase, 0);
                if (left < kChunk) qmask[q] &= (1ull << left) - 1ull;
                anymask |= qmask[q];
            }
        }
        if (cbase >= (int)lo + kChunk) {  // gather the next (shallower) chunk while this one is processed; it is always full
            nxid = nnid;
            if (cbase >= 2 * kChunk) nnid = a.point_list[range.x + (uint32_t)(cbase - 2 * kChunk) + (uint32_t)lane];
            const float4* g = reinterpret_cast<const float4*>(a.rec + nxid);
            nxa = g[0];
            nxb = g[1];
            nxc = g[2];
            if (REUSE && lane < 4) nxm = masks0[(size_t)((cbase - kChunk) >> 6) * 4 + lane];
        }
        __syncthreads();
        const int n = (int)min((uint32_t)kChunk, hi - (uint32_t)cbase);
        unsigned long long contributed = 0ull;   // wave-uniform: entries of this chunk that got sums
        while (anymask) {  // surviving entries, back to front: highest set bit first
            const int j = 63 - __builtin_clzll(anymask);
            anymask &= ~(1ull << j);
            const QSplat s = load_splat(s_rec[j]);
            const uint32_t pos = (uint32_t)(cbase + j);
            unsigned long long hit = 0ull;
#pragma unroll
            for (int q = 0; q < PPL; q++)
                if ((qmask[q] >> j) & 1ull) {
                    BwdEval e;
                    const bool valid = bwd_test(s, pxf[q], pyf[q], pos, pix[q], e);
                    // ballot of ONE compare is that compare's SGPR pair; of the conjunction it is a v_cndmask + v_cmp.
                    // `hit` only gates the reduction, so it may over-approximate: power > 0 (a degenerate conic) is
                    // left out, such an entry then reduces and stores the zeros it accumulated.
                    hit |= __builtin_amdgcn_ballot_w64(e.in_list) & __builtin_amdgcn_ballot_w64(e.visible);
                    if (valid) {
                        if (ABS) bwd_accumulate_abs(s, e, pix[q], sa);
                        bwd_accumulate(s, e, pix[q], sg);
                    }
                }
            if (hit != 0ull) {
                const float z = wave_reduce9(sg, lane);
                int joff = j * GS;
                asm("" : "+s"(joff));   // stays a scalar multiply + v_add (else: one quarter-rate v_mad_u64_u32)
                if (writer) s_grad_slot[joff] = z;
                if (ABS) {
                    const float z2 = wave_reduce2(sa.ax, sa.ay, lane);
                    if (lane < 2) s_grad[joff + kGradStride + lane] = z2;
                }
                contributed |= 1ull << j;
#ifndef R3_OLD_TRIP_FORMS
                {   // The nine sums are cleared by three broadcast LDS reads of zeros (2 x b128 + b32) instead of nine v_mov:
                    // the kernel is bound by VALU issue and the LDS pipe is not, the reads return ahead of the next entry's
                    // record (same queue, issued first), and no VGPR is added (the address register of s_rec serves).
                    // 33 -> 24 VALU per reduced entry; metric shape 1512 -> 1526 it/s (profiles/blend_inner_loop_ab.txt, visit 1).
                    typedef float v4f __attribute__((ext_vector_type(4)));
                    const volatile v4f __attribute__((address_space(3)))* zp =
                        (const volatile v4f __attribute__((address_space(3)))*)reinterpret_cast<float*>(s_zero);
                    const v4f z0 = zp[0], z1 = zp[1];
                    const float z2 = *(const volatile float __attribute__((address_space(3)))*)(zp + 2);
                    sg.sx = z0.x; sg.sy = z0.y; sg.sxx = z0.z; sg.sxy = z0.w;
                    sg.syy = z1.x; sg.sm = z1.y; sg.r = z1.z; sg.g = z1.w; sg.b = z2;
                    if (ABS) {   // the spare zeros of s_zero
                        const volatile float __attribute__((address_space(3)))* zf =
                            (const volatile float __attribute__((address_space(3)))*)(zp + 2);
                        sa.ax = zf[1];
                        sa.ay = zf[2];
                    }
                }
#else
                sg.sx = sg.sy = sg.sxx = sg.sxy = sg.syy = sg.sm = sg.r = sg.g = sg.b = 0.f;
                sa.ax = sa.ay = 0.f;
#endif
            }
        }
        __syncthreads();
        if (lane < n && ((contributed >> lane) & 1ull)) {
            // park the entry's sums in ITS slot of the per-pair slab: slot = first pair of the Gaussian + row-major
            // index of this tile inside the Gaussian's tile rect (exactly the emission order of binning.hip).
            // Plain stores, one owner per slot -- the per-Gaussian kernel adds a Gaussian's slots up in order, so
            // the backward has no float atomics and is bit-reproducible.  Only a 1-byte flag per pair is zeroed
            // before the pass (3.6 MB instead of the 131 MB slab); rows without flag are never read.
            const float4 c = s_rec[lane].c;
            const uint32_t rect_min = __float_as_uint(c.y), width = __float_as_uint(c.z) & 0xffffu;
            const uint32_t slot = __float_as_uint(c.w) + ((uint32_t)tile_y - (rect_min >> 16)) * width +
                                  ((uint32_t)tile_x - (rect_min & 0xffffu));
            float4* dst = reinterpret_cast<float4*>(a.pair_grad + (size_t)slot * kPairStride);   // 48-B row, 3 x 16 B
            const float* src = s_grad + lane * GS;
            SplatSums u;
            u.sx = src[0];
            u.sy = src[1];
            u.sxx = src[2];
            u.sxy = src[3];
            u.syy = src[4];
            u.sm = src[5];
            u.r = src[6];
            u.g = src[7];
            u.b = src[8];
            // moments -> gradients, once per (tile, entry); viewport factors of backward.cu:498-499 applied here
            const SplatGrad g = splat_grad_of(load_splat(s_rec[lane]), u);
            dst[0] = make_float4(g.mx * half_w, g.my * half_h, g.cA, g.cB);
            dst[1] = make_float4(g.cC, g.op, g.r, g.g);
            if (ABS) {
                SplatAbsSums ua;
                ua.ax = src[kGradStride];
                ua.ay = src[kGradStride + 1];
                float gax, gay;
                splat_abs_grad_of(load_splat(s_rec[lane]), ua, &gax, &gay);
                dst[2] = make_float4(g.b, gax * half_w, gay * half_h, 0.f);
            } else {
                dst[2] = make_float4(g.b, 0.f, 0.f, 0.f);
            }
            if (kPairStride >= 16) dst[3] = make_float4(0.f, 0.f, 0.f, 0.f);   // 64-byte rows: the whole burst is written
            a.pair_flag[slot] = 1;
        }
    }
    R3_TL_END(hi - lo)
}

#if defined(R3_TIMELINE) || defined(R3_TIMELINE_FWD)
extern "C" int r3dgs_debug_timeline(unsigned long long* host, int n)
{
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_timeline), sizeof(unsigned long long) * 4 * (size_t)n);
}
#endif

template <bool REUSE, bool ABS>
static void launch_bwd(uint32_t nblocks, uint32_t units_cap, BwdPassArgs* dst, const BwdPassArgs& v, hipStream_t s)
{
    if (v.blend.unit_order) {
        static const int lds_pad = env_int("R3DGS_BWD_LDS_PAD", 0, 0, 65536);
        // one workgroup per unit the pass MAY have (those beyond its count leave at once)
        hipLaunchKernelGGL((blend_bwd_kernel<4, REUSE, false, ABS>), dim3(units_cap), dim3(64), lds_pad, s, dst, v);
    } else {
        hipLaunchKernelGGL((blend_bwd_kernel<4, REUSE, true, ABS>), dim3(nblocks), dim3(64), 0, s, dst, v);
    }
}

void issue_blend_backward(const BwdPlan& p, BwdPassArgs* dst, const BwdPassArgs& v, hipStream_t s)
{
    // one wave per tile (PPL = 4): the per-pair gradient slab has exactly one owner per (tile, Gaussian)
    const uint32_t nblocks = (uint32_t)(p.gx * p.gy);   // == v.blend.nblocks
    if (p.absgrad) {
        if (v.blend.quad_masks)
            launch_bwd<true, true>(nblocks, p.units_cap, dst, v, s);
        else
            launch_bwd<false, true>(nblocks, p.units_cap, dst, v, s);
    } else if (v.blend.quad_masks) {
        launch_bwd<true, false>(nblocks, p.units_cap, dst, v, s);
    } else {
        launch_bwd<false, false>(nblocks, p.units_cap, dst, v, s);
    }
}

}  // namespace r3
