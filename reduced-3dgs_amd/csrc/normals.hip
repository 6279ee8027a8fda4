// normals.hip -- the surface-normal unit of include/r3dgs_normals.h: per-Gaussian view-space normals, the normal map of a depth
// map and the depth-normal consistency loss, each forward and backward.  Per-element arithmetic: normal_math.h.
//
// wave64, 256-thread workgroups, no float atomics, no host wait, no allocation; every kernel is bandwidth-bound.
//   gaussian normals   one lane per Gaussian; the view matrix and the camera position are staged in LDS once per workgroup.
//                      40 B read, 12 B written; backward 52 B read, 16 B written, the forward recomputed from the inputs.
//   depth normal       one lane per pixel of a 32 x 8 tile; the four neighbours' depth (and alpha) come through the cache.
//                      Per pixel 8 B read (depth, alpha) + 16 B with the loss (N, weight), 12 B written.  With the loss the
//                      workgroup leaves one double in its slot; ONE workgroup adds the slots in a fixed order.
//   backward           one lane per pixel of a 32 x 8 tile, RECOMPUTED from a staged tile: z of the tile and a two-pixel
//                      halo goes to LDS (36 x 12 doubles), then every centre of the tile and a one-pixel halo (34 x 10) is
//                      evaluated and leaves its four shares in LDS, then every pixel adds the shares its four neighbours hold
//                      for it, in a fixed order, and writes its own elements.  Nothing is kept between forward and backward.
//                      Per pixel: 8 B (depth, alpha) x 1.69 (halo) + 16 B (N, weight) or 12 B (upstream) x 1.33 read,
//                      up to 20 B written (dL/ddepth, dL/dalpha, dL/dN).
#include "../../include/r3dgs_normals.h"

#include "common.h"
#include "normal_math.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTileW = 32, kTileH = 8;
constexpr int kZW = kTileW + 4, kZH = kTileH + 4;   // z: the tile and a two-pixel halo
constexpr int kCW = kTileW + 2, kCH = kTileH + 2;   // centres: the tile and a one-pixel halo
constexpr int kRing = kCW * kCH - kBlock;           // the centres of the halo ring
constexpr long long kMaxP = 1LL << 30;
constexpr long long kMaxPixels = 1LL << 30;
static_assert(kTileW * kTileH == kBlock, "one lane per pixel of a tile");
static_assert(kRing <= kBlock, "the ring is evaluated in one more round");
static_assert(r3::kNormalAlphaMin == R3DGS_NORMAL_ALPHA_MIN && r3::kNormalCrossMin == R3DGS_NORMAL_CROSS_MIN, "the header's constants");

struct __attribute__((packed, aligned(4))) Row3 {
    float v[3];
};

inline long long blocks_of(long long P) { return (P + kBlock - 1) / kBlock; }

template <bool RAW, bool BWD>
__global__ __launch_bounds__(kBlock) void gaussian_normals_kernel(int P, const float* __restrict__ means3D,
                                                                  const float* __restrict__ scales,
                                                                  const float* __restrict__ rotations,
                                                                  const float* __restrict__ view, const float* __restrict__ campos,
                                                                  const float* __restrict__ g, float* __restrict__ out)
{
    __shared__ float s_cam[19];
    if (threadIdx.x < 16) s_cam[threadIdx.x] = view[threadIdx.x];
    if (threadIdx.x >= 16 && threadIdx.x < 19) s_cam[threadIdx.x] = campos[threadIdx.x - 16];
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (size_t)P) return;
    const Row3 m = reinterpret_cast<const Row3*>(means3D)[i];
    const Row3 s = reinterpret_cast<const Row3*>(scales)[i];
    const float4 q4 = reinterpret_cast<const float4*>(rotations)[i];
    const float q[4] = {q4.x, q4.y, q4.z, q4.w};
    if (BWD) {
        const Row3 gi = reinterpret_cast<const Row3*>(g)[i];
        float dq[4];
        r3::gaussian_normal_bwd_one(s_cam, s_cam + 16, m.v, s.v, q, RAW, gi.v, dq);
        reinterpret_cast<float4*>(out)[i] = make_float4(dq[0], dq[1], dq[2], dq[3]);
    } else {
        Row3 n;
        r3::gaussian_normal_one(s_cam, s_cam + 16, m.v, s.v, q, RAW, n.v);
        reinterpret_cast<Row3*>(out)[i] = n;
    }
}

// ---- depth normals ------------------------------------------------------------------------------------------------------------

struct ImageArgs {
    int H, W;
    float tan_fovx, tan_fovy;
    const float* depth;
    const float* alpha;
    const float* normal_map;
    const float* weight;
    int scale_by_alpha;
};

__device__ __forceinline__ double z_at(const float* depth, const float* alpha, size_t p)
{
    return r3::normal_pixel_z(depth[p], alpha ? alpha[p] : 1.f, alpha != nullptr);
}

__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

__global__ __launch_bounds__(kBlock) void depth_normal_kernel(const ImageArgs a, float* __restrict__ surf, double* __restrict__ slots)
{
    __shared__ double s_red[kBlock / 64];
    const int tid = threadIdx.x;
    const int x = blockIdx.x * kTileW + (tid & (kTileW - 1)), y = blockIdx.y * kTileH + tid / kTileW;
    const bool in = x < a.W && y < a.H;
    const size_t plane = (size_t)a.H * a.W, p = (size_t)y * a.W + x;
    double term = 0.0;
    if (in) {
        double n[3] = {0.0, 0.0, 0.0};
        if (x >= 1 && x <= a.W - 2 && y >= 1 && y <= a.H - 2) {
            const r3::NormalRays r = r3::normal_rays(a.W, a.H, a.tan_fovx, a.tan_fovy);
            const r3::DepthNormal o = r3::depth_normal_one(z_at(a.depth, a.alpha, p - a.W), z_at(a.depth, a.alpha, p + a.W),
                                                           z_at(a.depth, a.alpha, p - 1), z_at(a.depth, a.alpha, p + 1),
                                                           r.x0 + x * r.dx, r.y0 + y * r.dy, r.dx, r.dy);
            n[0] = o.n[0], n[1] = o.n[1], n[2] = o.n[2];
        }
        surf[p] = (float)n[0];
        surf[plane + p] = (float)n[1];
        surf[2 * plane + p] = (float)n[2];
        if (a.normal_map) {
            const float N[3] = {a.normal_map[p], a.normal_map[plane + p], a.normal_map[2 * plane + p]};
            const double w = a.weight ? (double)a.weight[p] : 1.0;
            const double s = a.scale_by_alpha && a.alpha ? (double)a.alpha[p] : 1.0;
            term = r3::normal_loss_term(w, s, N, n);
        }
    }
    if (!slots) return;   // (uniform: a kernel argument)
    term = wave_sum(term);
    if ((tid & 63) == 0) s_red[tid >> 6] = term;
    __syncthreads();
    if (tid == 0) slots[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

// One workgroup: thread-strided double sums of the slots and a fixed tree.
__global__ __launch_bounds__(kBlock) void loss_finish_kernel(long long nb, double pixels, const double* __restrict__ slots,
                                                             float* __restrict__ loss)
{
    __shared__ double buf[kBlock];
    double s = 0.0;
    for (long long b = threadIdx.x; b < nb; b += kBlock) s += slots[b];
    buf[threadIdx.x] = s;
    __syncthreads();
    for (int half = kBlock / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) buf[threadIdx.x] += buf[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(buf[0] / pixels);
}

struct ImageGrads {
    const float* g_loss;
    const float* g_surf;
    float* d_depth;
    float* d_alpha;
    float* d_normal;
};

__global__ __launch_bounds__(kBlock) void depth_normal_bwd_kernel(const ImageArgs a, const ImageGrads o)
{
    __shared__ double s_z[kZH][kZW];
    __shared__ double s_to[4][kCH][kCW];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const size_t plane = (size_t)a.H * a.W;
    for (int k = tid; k < kZW * kZH; k += kBlock) {
        const int ly = k / kZW, lx = k - ly * kZW;
        const int gx = x0 + lx - 2, gy = y0 + ly - 2;
        const bool in = gx >= 0 && gx < a.W && gy >= 0 && gy < a.H;
        s_z[ly][lx] = in ? z_at(a.depth, a.alpha, (size_t)gy * a.W + gx) : 0.0;
    }
    __syncthreads();
    const r3::NormalRays r = r3::normal_rays(a.W, a.H, a.tan_fovx, a.tan_fovy);
    // upstream of the loss, per unit of N: dL/dn = -g w s N / (H W), dL/dN = -g w s n / (H W)
    const double gl = a.normal_map && o.g_loss ? (double)o.g_loss[0] / (double)plane : 0.0;
    double n_own[3] = {0.0, 0.0, 0.0}, ws_own = 0.0;
    // centre (lx, ly) of the 34 x 10 grid is pixel (x0 + lx - 1, y0 + ly - 1) and z cell [ly + 1][lx + 1]
    auto centre = [&](int lx, int ly, bool own) {
        const int gx = x0 + lx - 1, gy = y0 + ly - 1;
        double to[4] = {0.0, 0.0, 0.0, 0.0};
        if (gx >= 1 && gx <= a.W - 2 && gy >= 1 && gy <= a.H - 2) {
            const size_t p = (size_t)gy * a.W + gx;
            const double rx = r.x0 + gx * r.dx, ry = r.y0 + gy * r.dy;
            const r3::DepthNormal d = r3::depth_normal_one(s_z[ly][lx + 1], s_z[ly + 2][lx + 1], s_z[ly + 1][lx], s_z[ly + 1][lx + 2],
                                                           rx, ry, r.dx, r.dy);
            double g[3] = {0.0, 0.0, 0.0};
            if (o.g_surf) g[0] = o.g_surf[p], g[1] = o.g_surf[plane + p], g[2] = o.g_surf[2 * plane + p];
            if (gl != 0.0) {
                const double w = a.weight ? (double)a.weight[p] : 1.0;
                const double s = a.scale_by_alpha && a.alpha ? (double)a.alpha[p] : 1.0;
                const double f = -gl * w * s;
                g[0] += f * a.normal_map[p], g[1] += f * a.normal_map[plane + p], g[2] += f * a.normal_map[2 * plane + p];
                if (own) ws_own = f;
            }
            if (own) n_own[0] = d.n[0], n_own[1] = d.n[1], n_own[2] = d.n[2];
            r3::depth_normal_bwd_one(d, rx, ry, r.dx, r.dy, g, to);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) s_to[k][ly][lx] = to[k];
    };
    const int tx = tid & (kTileW - 1), ty = tid / kTileW;
    centre(tx + 1, ty + 1, true);
    if (tid < kRing) {
        int lx, ly;
        if (tid < kCW) lx = tid, ly = 0;
        else if (tid < 2 * kCW) lx = tid - kCW, ly = kCH - 1;
        else if (tid < 2 * kCW + kTileH) lx = 0, ly = tid - 2 * kCW + 1;
        else lx = kCW - 1, ly = tid - 2 * kCW - kTileH + 1;
        centre(lx, ly, false);
    }
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * a.W + x;
    const int lx = tx + 1, ly = ty + 1;
    // this pixel is: below the centre above it, above the centre below it, right of the centre to its left, left of the one to its right
    const double gz = ((s_to[0][ly - 1][lx] + s_to[1][ly + 1][lx]) + s_to[2][ly][lx - 1]) + s_to[3][ly][lx + 1];
    double d_depth = gz, d_alpha = 0.0;
    if (a.alpha) {
        const float al = a.alpha[p];
        if (r3::normal_alpha_live(al)) {
            d_depth = gz / (double)al;
            d_alpha = -gz * (double)a.depth[p] / ((double)al * (double)al);
        } else {
            d_depth = 0.0;
        }
    }
    if (o.d_depth) o.d_depth[p] = (float)d_depth;
    if (o.d_alpha) o.d_alpha[p] = (float)d_alpha;
    if (o.d_normal) {
        o.d_normal[p] = (float)(ws_own * n_own[0]);
        o.d_normal[plane + p] = (float)(ws_own * n_own[1]);
        o.d_normal[2 * plane + p] = (float)(ws_own * n_own[2]);
    }
}

void checked_gaussians(const char* what, int P, const float* means3D, const float* scales, const float* rotations,
                       const float* view, const float* campos, const float* extra, const float* out)
{
    const std::string w(what);
    if (P > kMaxP) throw r3::Error(w + ": P exceeds 2^30");
    if (!means3D || !scales || !rotations || !view || !campos || !extra || !out) throw r3::Error(w + ": a tensor is NULL");
    if ((uintptr_t)rotations % 16) throw r3::Error(w + ": rotations must be 16-byte aligned");
    if ((uintptr_t)means3D % 4 || (uintptr_t)scales % 4 || (uintptr_t)view % 4 || (uintptr_t)campos % 4 || (uintptr_t)extra % 4 ||
        (uintptr_t)out % 4)
        throw r3::Error(w + ": a tensor is not 4-byte aligned");
}

ImageArgs checked_image(const char* what, int H, int W, float tan_fovx, float tan_fovy, const float* depth, const float* alpha,
                        const float* normal_map, const float* weight, int scale_by_alpha)
{
    const std::string w(what);
    if ((long long)H * W > kMaxPixels) throw r3::Error(w + ": H * W exceeds 2^30");
    if (!(tan_fovx > 0.f) || !(tan_fovy > 0.f)) throw r3::Error(w + ": tan_fovx and tan_fovy must be positive");
    if (!depth) throw r3::Error(w + ": depth is NULL");
    if (weight && !normal_map) throw r3::Error(w + ": pixel_weight without normal_map");
    if ((uintptr_t)depth % 4 || (uintptr_t)alpha % 4 || (uintptr_t)normal_map % 4 || (uintptr_t)weight % 4)
        throw r3::Error(w + ": a tensor is not 4-byte aligned");
    ImageArgs a;
    a.H = H;
    a.W = W;
    a.tan_fovx = tan_fovx;
    a.tan_fovy = tan_fovy;
    a.depth = depth;
    a.alpha = alpha;
    a.normal_map = normal_map;
    a.weight = weight;
    a.scale_by_alpha = scale_by_alpha ? 1 : 0;
    return a;
}

inline dim3 tiles_of(int H, int W) { return dim3((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH), 1); }

}  // namespace

extern "C" {

int r3dgs_gaussian_normals(int P, const float* means3D, const float* scales, const float* rotations, int raw,
                           const float* viewmatrix, const float* campos, float* normals, void* stream)
{
    return r3::guarded_call([&]() {
        if (P <= 0) return 0;
        checked_gaussians("gaussian_normals", P, means3D, scales, rotations, viewmatrix, campos, means3D, normals);
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (raw)
            gaussian_normals_kernel<true, false><<<(unsigned)blocks_of(P), kBlock, 0, s>>>(P, means3D, scales, rotations, viewmatrix, campos, nullptr, normals);
        else
            gaussian_normals_kernel<false, false><<<(unsigned)blocks_of(P), kBlock, 0, s>>>(P, means3D, scales, rotations, viewmatrix, campos, nullptr, normals);
        r3::check_launch("gaussian normals", s, false);
        return 0;
    });
}

int r3dgs_gaussian_normals_backward(int P, const float* means3D, const float* scales, const float* rotations, int raw,
                                    const float* viewmatrix, const float* campos, const float* dL_dnormals,
                                    float* dL_drotations, void* stream)
{
    return r3::guarded_call([&]() {
        if (P <= 0) return 0;
        checked_gaussians("gaussian_normals_backward", P, means3D, scales, rotations, viewmatrix, campos, dL_dnormals, dL_drotations);
        if ((uintptr_t)dL_drotations % 16) throw r3::Error("gaussian_normals_backward: dL_drotations must be 16-byte aligned");
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (raw)
            gaussian_normals_kernel<true, true><<<(unsigned)blocks_of(P), kBlock, 0, s>>>(P, means3D, scales, rotations, viewmatrix, campos, dL_dnormals, dL_drotations);
        else
            gaussian_normals_kernel<false, true><<<(unsigned)blocks_of(P), kBlock, 0, s>>>(P, means3D, scales, rotations, viewmatrix, campos, dL_dnormals, dL_drotations);
        r3::check_launch("gaussian normals backward", s, false);
        return 0;
    });
}

size_t r3dgs_depth_normal_workspace_bytes(int H, int W)
{
    if (H <= 0 || W <= 0 || (long long)H * W > kMaxPixels) return 0;
    const dim3 g = tiles_of(H, W);
    return (size_t)g.x * g.y * sizeof(double);
}

int r3dgs_depth_normal(int H, int W, float tan_fovx, float tan_fovy, const float* depth, const float* alpha,
                       const float* normal_map, const float* pixel_weight, int scale_by_alpha, float* surf_normal, float* loss,
                       char* workspace, void* stream)
{
    return r3::guarded_call([&]() {
        if (H <= 0 || W <= 0) return 0;
        const ImageArgs a = checked_image("depth_normal", H, W, tan_fovx, tan_fovy, depth, alpha, normal_map, pixel_weight, scale_by_alpha);
        if (!surf_normal || (uintptr_t)surf_normal % 4) throw r3::Error("depth_normal: surf_normal is NULL or not 4-byte aligned");
        if (normal_map && (!loss || (uintptr_t)loss % 4 || !workspace || (uintptr_t)workspace % alignof(double)))
            throw r3::Error("depth_normal: with normal_map, loss and an 8-byte aligned workspace are needed");
        hipStream_t s = static_cast<hipStream_t>(stream);
        const dim3 g = tiles_of(H, W);
        double* slots = normal_map ? reinterpret_cast<double*>(workspace) : nullptr;
        depth_normal_kernel<<<g, kBlock, 0, s>>>(a, surf_normal, slots);
        r3::check_launch("depth normal", s, false);
        if (slots) {
            loss_finish_kernel<<<1, kBlock, 0, s>>>((long long)g.x * g.y, (double)H * (double)W, slots, loss);
            r3::check_launch("depth normal loss finish", s, false);
        }
        return 0;
    });
}

int r3dgs_depth_normal_backward(int H, int W, float tan_fovx, float tan_fovy, const float* depth, const float* alpha,
                                const float* normal_map, const float* pixel_weight, int scale_by_alpha, const float* dL_dloss,
                                const float* dL_dsurf, float* dL_ddepth, float* dL_dalpha, float* dL_dnormal_map, void* stream)
{
    return r3::guarded_call([&]() {
        if (H <= 0 || W <= 0) return 0;
        const ImageArgs a = checked_image("depth_normal_backward", H, W, tan_fovx, tan_fovy, depth, alpha, normal_map, pixel_weight,
                                          scale_by_alpha);
        if (dL_dloss && !normal_map) throw r3::Error("depth_normal_backward: dL_dloss without normal_map");
        if (dL_dalpha && !alpha) throw r3::Error("depth_normal_backward: dL_dalpha without alpha");
        if (dL_dnormal_map && !normal_map) throw r3::Error("depth_normal_backward: dL_dnormal_map without normal_map");
        if ((uintptr_t)dL_dloss % 4 || (uintptr_t)dL_dsurf % 4 || (uintptr_t)dL_ddepth % 4 || (uintptr_t)dL_dalpha % 4 ||
            (uintptr_t)dL_dnormal_map % 4)
            throw r3::Error("depth_normal_backward: a tensor is not 4-byte aligned");
        if (!dL_ddepth && !dL_dalpha && !dL_dnormal_map) return 0;
        const ImageGrads o{dL_dloss, dL_dsurf, dL_ddepth, dL_dalpha, dL_dnormal_map};
        hipStream_t s = static_cast<hipStream_t>(stream);
        depth_normal_bwd_kernel<<<tiles_of(H, W), kBlock, 0, s>>>(a, o);
        r3::check_launch("depth normal backward", s, false);
        return 0;
    });
}

}  // extern "C"
