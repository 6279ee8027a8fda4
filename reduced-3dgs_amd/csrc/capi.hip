// capi.hip -- the extern "C" boundary declared in include/r3dgs_rasterizer.h and include/r3dgs_quantised.h: every entry
// point checks what only it can check, packs its arguments into a call (pass_driver.h) and hands it to the pass driver
// (pass_driver.hip), which plans, fills and issues the pass; exceptions become r3dgs_last_error() here.  Also
// Rasterizer::markVisible (rasterizer_impl.cu:149-161) and the export / size queries over a pass's blobs.
#include "../../include/r3dgs_rasterizer.h"
#include "../../include/r3dgs_quantised.h"

#include <string>

#include "pass_driver.h"
#include "quant_math.h"
#include "reserve_advice.h"

namespace {

using namespace r3;

thread_local std::string g_last_error;

// Every entry point's body: clears r3dgs_last_error(), and turns an exception into the message and the entry point's
// failure value (-1 for the int / long long ones, 0 for the *_bytes queries).
template <class F, class R = decltype(std::declval<F>()())>
R guarded(F&& f, R failure = R(-1))
{
    try {
        g_last_error.clear();
        return f();
    } catch (const std::exception& e) {
        g_last_error = e.what();
        return failure;
    }
}

#define R3_FWD_CALL(coeffs, perband, cumsum, Mval)                                                                      \
    FwdCall c;                                                                                                          \
    c.P = P;                                                                                                            \
    c.D = D;                                                                                                            \
    c.M = (Mval);                                                                                                       \
    c.coeffsNum = (coeffs);                                                                                             \
    c.perBand = (perband);                                                                                              \
    c.cumSum = (cumsum);                                                                                                \
    c.background = background;                                                                                          \
    c.width = width;                                                                                                    \
    c.height = height;                                                                                                  \
    c.means3D = means3D;                                                                                                \
    c.shs = shs;                                                                                                        \
    c.colors_precomp = colors_precomp;                                                                                  \
    c.opacities = opacities;                                                                                            \
    c.scales = scales;                                                                                                  \
    c.scale_modifier = scale_modifier;                                                                                  \
    c.rotations = rotations;                                                                                            \
    c.cov3D_precomp = cov3D_precomp;                                                                                    \
    c.viewmatrix = viewmatrix;                                                                                          \
    c.projmatrix = projmatrix;                                                                                          \
    c.cam_pos = cam_pos;                                                                                                \
    c.tan_fovx = tan_fovx;                                                                                              \
    c.tan_fovy = tan_fovy;                                                                                              \
    c.out_color = out_color;                                                                                            \
    c.out_touched_pixels = out_touched_pixels;                                                                          \
    c.out_transmittance = out_transmittance;                                                                            \
    c.radii = radii;                                                                                                    \
    c.calculate_mean_transmittance = calculate_mean_transmittance;                                                      \
    c.debug = debug;                                                                                                    \
    c.shs_rest = nullptr;                                                                                               \
    c.raw = 0;                                                                                                          \
    c.stream = static_cast<hipStream_t>(stream)

void check_ragged(const float* colors_precomp, int bandsNum, const int*& coeffsNum, const int*& perBand, const int*& cumSum)
{
    if (!colors_precomp) {
        if (bandsNum != 4) throw Error("ragged SH path expects 4 bands (degrees 0..3)");
        if (!coeffsNum || !perBand || !cumSum)
            throw Error("ragged SH path needs coeffsNum / perBandPrimitiveCount / cumSumPrimitiveCount");
    } else {
        coeffsNum = perBand = cumSum = nullptr;
    }
}

}  // namespace

int r3::guarded_call(const std::function<int()>& f) { return guarded(f); }

extern "C" {

const char* r3dgs_version(void) { return "r3dgs-hip gfx950 0.4"; }
const char* r3dgs_last_error(void) { return g_last_error.c_str(); }

// The temp-storage part of the geometry blob comes from a rocPRIM query, which needs a visible GPU;
// without one it returns 0 and sets r3dgs_last_error().
size_t r3dgs_geometry_bytes(int P)
{
    return guarded([&]() { return r3::required_bytes<r3::GeomState>((size_t)P, cached_depth_temp((size_t)(P > 0 ? P : 1))); },
                   (size_t)0);
}
size_t r3dgs_geometry_bytes_lean(int P)
{
    return guarded([&]() { return geometry_blob_bytes((size_t)P, cached_depth_temp((size_t)(P > 0 ? P : 1)), true); }, (size_t)0);
}
size_t r3dgs_binning_bytes(int P, int width, int height, int reserve)
{
    return guarded(
        [&]() {
            const TileGrid grid = grid_of(width, height);
            return required_bytes<BinState>((size_t)(reserve > 0 ? reserve : 1), pair_layout(P, grid.n()).wide, grid);
        },
        (size_t)0);
}
size_t r3dgs_image_bytes(int width, int height)
{
    return required_bytes<ImageState>((size_t)width * height, grid_of(width, height).n());
}
int r3dgs_binning_capacity(int P, int width, int height, size_t bytes)
{
    return guarded([&]() {
        const TileGrid grid = grid_of(width, height);
        const PairLayout l = pair_layout(P, grid.n());
        if (required_bytes<BinState>((size_t)1, l.wide, grid) > bytes) return 0;
        // largest R whose layout fits: every array size is monotone in R, so any R with the same total has the same
        // offsets -- the capacity recovered from a blob's size reproduces the carve the forward used
        long long lo = 1, hi = 0x7fffffffLL;
        while (lo < hi) {
            const long long mid = (lo + hi + 1) / 2;
            if (required_bytes<BinState>((size_t)mid, l.wide, grid) <= bytes)
                lo = mid;
            else
                hi = mid - 1;
        }
        return (int)lo;
    });
}

int r3dgs_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                       unsigned char* present, void* stream)
{
    (void)projmatrix;  // unused by the reference too (rasterizer_impl.cu:62-74)
    return guarded([&]() {
        if (P <= 0) return 0;
        if (!means3D || !viewmatrix || !present) throw r3::Error("a required pointer is NULL");
        hipStream_t s = static_cast<hipStream_t>(stream);
        r3::launch_mark_visible(P, means3D, viewmatrix, reinterpret_cast<bool*>(present), s);
        r3::check_launch("mark_visible", s, false);
        return 0;
    });
}

int r3dgs_forward(r3dgs_alloc_fn geometryBuffer, void* geometry_user, r3dgs_alloc_fn binningBuffer, void* binning_user,
                  r3dgs_alloc_fn imageBuffer, void* image_user, int P, const int* D, int M, const float* background,
                  int width, int height, const float* means3D, const float* shs, const float* colors_precomp,
                  const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                  const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                  float tan_fovx, float tan_fovy, int prefiltered, float* out_color, int* out_touched_pixels,
                  float* out_transmittance, int* radii, int calculate_mean_transmittance, int debug, void* stream)
{
    (void)prefiltered;
    return guarded([&]() {
        R3_FWD_CALL(nullptr, nullptr, nullptr, M);
        return forward_exact({geometryBuffer, geometry_user, binningBuffer, binning_user, imageBuffer, image_user}, c);
    });
}

int r3dgs_inference_forward(r3dgs_alloc_fn geometryBuffer, void* geometry_user, r3dgs_alloc_fn binningBuffer,
                            void* binning_user, r3dgs_alloc_fn imageBuffer, void* image_user, int P, const int* D,
                            int bandsNum, const int* coeffsNum, const int* perBandPrimitiveCount,
                            const int* cumSumPrimitiveCount, const float* background, int width, int height,
                            const float* means3D, const float* shs, const float* colors_precomp,
                            const float* opacities, const float* scales, float scale_modifier,
                            const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                            const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                            int prefiltered, float* out_color, int* out_touched_pixels, float* out_transmittance,
                            int* radii, int calculate_mean_transmittance, int debug, void* stream)
{
    (void)prefiltered;
    return guarded([&]() {
        check_ragged(colors_precomp, bandsNum, coeffsNum, perBandPrimitiveCount, cumSumPrimitiveCount);
        R3_FWD_CALL(coeffsNum, perBandPrimitiveCount, cumSumPrimitiveCount, 16);
        return forward_exact({geometryBuffer, geometry_user, binningBuffer, binning_user, imageBuffer, image_user}, c);
    });
}

int r3dgs_reserve_hint(int P, int width, int height)
{
    return guarded([&]() { return (int)reserve_hint(P, width, height, nullptr); });
}

int r3dgs_reserve_hint_view(int P, int width, int height, const float* viewmatrix)
{
    return guarded([&]() { return (int)reserve_hint(P, width, height, viewmatrix); });
}

void r3dgs_reserve_forget_view(const float* viewmatrix) { reserve_forget_view(viewmatrix); }

long long r3dgs_forward_reserved(char* geom_buffer, char* binning_buffer, char* image_buffer, int reserve, int P,
                                 const int* D, int M, const float* background, int width, int height,
                                 const float* means3D, const float* shs, const float* colors_precomp,
                                 const float* opacities, const float* scales, float scale_modifier,
                                 const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                                 const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                                 int prefiltered, float* out_color, int* out_touched_pixels, float* out_transmittance,
                                 int* radii, int calculate_mean_transmittance, int debug, void* stream)
{
    (void)prefiltered;
    return guarded([&]() {
        R3_FWD_CALL(nullptr, nullptr, nullptr, M);
        return forward_reserved({geom_buffer, binning_buffer, image_buffer}, reserve, c);
    });
}

long long r3dgs_inference_forward_reserved(char* geom_buffer, char* binning_buffer, char* image_buffer, int reserve,
                                           int P, const int* D, int bandsNum, const int* coeffsNum,
                                           const int* perBandPrimitiveCount, const int* cumSumPrimitiveCount,
                                           const float* background, int width, int height, const float* means3D,
                                           const float* shs, const float* colors_precomp, const float* opacities,
                                           const float* scales, float scale_modifier, const float* rotations,
                                           const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                                           const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered,
                                           float* out_color, int* out_touched_pixels, float* out_transmittance,
                                           int* radii, int calculate_mean_transmittance, int debug, void* stream)
{
    (void)prefiltered;
    return guarded([&]() {
        check_ragged(colors_precomp, bandsNum, coeffsNum, perBandPrimitiveCount, cumSumPrimitiveCount);
        R3_FWD_CALL(coeffsNum, perBandPrimitiveCount, cumSumPrimitiveCount, 16);
        return forward_reserved({geom_buffer, binning_buffer, image_buffer}, reserve, c);
    });
}

int r3dgs_pass_query(long long ticket, int wait, int* num_rendered, int* visible, int* reserve, int* flags)
{
    return guarded([&]() {
        const volatile PassInfo* info = pass_info(ticket, wait);
        if (!info) return 0;
        const uint32_t R = info->num_rendered, pairs = info->pairs, cap = info->reserve;
        const uint32_t n = (uint32_t)ticket_number((uint64_t)ticket);
        if (num_rendered) *num_rendered = (int)(R > 0x7fffffffu ? 0x7fffffffu : R);
        if (visible) *visible = (int)info->visible;
        if (reserve) *reserve = cap == 0xFFFFFFFFu ? -1 : (int)cap;
        // the depth-bucket hint is stamped by a later kernel of the pass than the header: reported once it is there
        if (flags) *flags = (cap != 0xFFFFFFFFu && pairs > cap ? R3DGS_PASS_TRUNCATED : 0) |
                            (info->sort_seq == n && info->sort_overflow ? R3DGS_PASS_DEPTH_BUCKET_OVERFLOW : 0);
        return 1;
    });
}

int r3dgs_pass_pairs(long long ticket, int wait)
{
    return guarded([&]() {
        const volatile PassInfo* info = pass_info(ticket, wait);
        if (!info) throw Error("pass not published yet");
        const uint32_t pairs = info->pairs;
        return (int)(pairs > 0x7fffffffu ? 0x7fffffffu : pairs);
    });
}

int r3dgs_forward_pairs(void) { return last_forward_pairs(); }

int r3dgs_set_tight_rects(int on) { return g_tight_rects.set(on); }   // on < 0: query only

void r3dgs_forward_hint(int will_backward) { set_forward_trains(will_backward ? 1 : 0); }

int r3dgs_set_sh_cache(int on) { return g_sh_cache.set(on); }   // on < 0: query only

int r3dgs_set_f64_chain(int on) { return g_f64_chain.set(on); }   // on < 0: query only

int r3dgs_set_bwd_segments(int on) { return g_bwd_segments.set(on); }   // on < 0: query only

int r3dgs_set_tile_order(int on) { return g_tile_order.set(on); }   // on < 0: query only

int r3dgs_export_rects(int P, char* geom_buffer, unsigned short* rects, void* stream)
{
    return guarded([&]() {
        using namespace r3;
        if (P <= 0) return 0;
        if (!geom_buffer || !rects) throw Error("a required pointer is NULL");
        GeomState geom = GeomState::carve(geom_buffer, (size_t)P, cached_depth_temp((size_t)P));
        R3_HIP(hipMemcpyAsync(rects, geom.rect, sizeof(ushort4) * (size_t)P, hipMemcpyDeviceToDevice,
                              static_cast<hipStream_t>(stream)));
        return 0;
    });
}

void r3dgs_reserve_forget(void) { reserve_forget_all(); }

long long r3dgs_reserve_overflow_events(int* last_num_rendered, int* last_reserve)
{
    return reserve_overflow_events(last_num_rendered, last_reserve);
}

// BwdCall's fields are the parameter list of r3dgs_backward, in this order, with the three blobs as one
static BwdCall backward_call(int P, const int* D, int M, int R, const float* background, int width, int height,
                             const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                             float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                             const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                             char* geom_buffer, char* binning_buffer, char* image_buffer, const float* dL_dpix, float* dL_dmean2D,
                             float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D,
                             float* dL_dsh, float* dL_dscale, float* dL_drot, float lambda_sh_sparsity, int debug, void* stream)
{
    return {P, D, M, R, background, width, height, means3D, shs, colors_precomp, scales, scale_modifier,
            rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii,
            {geom_buffer, binning_buffer, image_buffer}, dL_dpix, dL_dmean2D, dL_dconic, dL_dopacity,
            dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, lambda_sh_sparsity, debug,
            static_cast<hipStream_t>(stream), nullptr, nullptr, 0};
}

static void ask_absgrad(BwdCall& c, float* dL_dmean2D_abs, float* abs_workspace, size_t abs_workspace_floats)
{
    c.absgrad = 1;
    c.dL_dmean2D_abs = dL_dmean2D_abs;
    c.abs_workspace = abs_workspace;
    c.abs_workspace_floats = abs_workspace_floats;
}

int r3dgs_backward(int P, const int* D, int M, int R, const float* background, int width, int height,
                   const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                   float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                   const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                   char* geom_buffer, char* binning_buffer, char* image_buffer, const float* dL_dpix, float* dL_dmean2D,
                   float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D,
                   float* dL_dsh, float* dL_dscale, float* dL_drot, float lambda_sh_sparsity, int debug, void* stream)
{
    return guarded([&]() {
        return backward_pass(backward_call(P, D, M, R, background, width, height, means3D, shs, colors_precomp, scales,
                                           scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx,
                                           tan_fovy, radii, geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_dmean2D,
                                           dL_dconic, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot,
                                           lambda_sh_sparsity, debug, stream));
    });
}

size_t r3dgs_absgrad_workspace_floats(int R) { return r3::absgrad_workspace_floats((size_t)(R > 0 ? R : 1)); }

int r3dgs_backward_absgrad(int P, const int* D, int M, int R, const float* background, int width, int height,
                           const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                           float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                           const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                           char* geom_buffer, char* binning_buffer, char* image_buffer, const float* dL_dpix, float* dL_dmean2D,
                           float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D,
                           float* dL_dsh, float* dL_dscale, float* dL_drot, float lambda_sh_sparsity, int debug, void* stream,
                           float* dL_dmean2D_abs, float* abs_workspace, size_t abs_workspace_floats)
{
    return guarded([&]() {
        BwdCall c = backward_call(P, D, M, R, background, width, height, means3D, shs, colors_precomp, scales, scale_modifier,
                                  rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii,
                                  geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_dmean2D, dL_dconic, dL_dopacity,
                                  dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, lambda_sh_sparsity, debug, stream);
        ask_absgrad(c, dL_dmean2D_abs, abs_workspace, abs_workspace_floats);
        return backward_pass(c);
    });
}

// ---- the raw-parameter entry points (include/r3dgs_rasterizer.h) ------------------------------------------------------
static void check_params(int P, const int* D, int M, const float* features_dc, const float* features_rest,
                         const float* scaling_raw, const float* rotation_raw)
{
    if (P <= 0) return;
    if (M < 1 || M > 16) throw r3::Error("SH coefficient count M must be in [1,16]");
    if (!features_dc) throw r3::Error("raw-parameter path: features_dc is NULL");
    if ((features_rest == nullptr) != (M == 1))
        throw r3::Error("raw-parameter path: features_rest must be [P,M-1,3] (NULL iff M == 1)");
    if (!D) throw r3::Error("per-Gaussian degrees must be provided with SHs");
    if (!scaling_raw || !rotation_raw) throw r3::Error("raw-parameter path: scaling and rotation must be provided");
}

#define R3_PARAMS_CALL()                                                                                                \
    const float* shs = features_dc;                                                                                     \
    const float* colors_precomp = nullptr;                                                                              \
    const float* cov3D_precomp = nullptr;                                                                               \
    const float* scales = scaling_raw;                                                                                  \
    const float* rotations = rotation_raw;                                                                              \
    R3_FWD_CALL(nullptr, nullptr, nullptr, M);                                                                          \
    c.shs_rest = features_rest;                                                                                         \
    c.raw = 1

int r3dgs_forward_params(r3dgs_alloc_fn geometryBuffer, void* geometry_user, r3dgs_alloc_fn binningBuffer, void* binning_user,
                         r3dgs_alloc_fn imageBuffer, void* image_user, int P, const int* D, int M, const float* background,
                         int width, int height, const float* means3D, const float* features_dc, const float* features_rest,
                         const float* opacities, const float* scaling_raw, float scale_modifier, const float* rotation_raw,
                         const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                         int prefiltered, float* out_color, int* out_touched_pixels, float* out_transmittance, int* radii,
                         int calculate_mean_transmittance, int debug, void* stream)
{
    (void)prefiltered;
    return guarded([&]() {
        check_params(P, D, M, features_dc, features_rest, scaling_raw, rotation_raw);
        R3_PARAMS_CALL();
        return forward_exact({geometryBuffer, geometry_user, binningBuffer, binning_user, imageBuffer, image_user}, c);
    });
}

long long r3dgs_forward_params_reserved(char* geom_buffer, char* binning_buffer, char* image_buffer, int reserve, int P,
                                        const int* D, int M, const float* background, int width, int height,
                                        const float* means3D, const float* features_dc, const float* features_rest,
                                        const float* opacities, const float* scaling_raw, float scale_modifier,
                                        const float* rotation_raw, const float* viewmatrix, const float* projmatrix,
                                        const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color,
                                        int* out_touched_pixels, float* out_transmittance, int* radii,
                                        int calculate_mean_transmittance, int debug, void* stream)
{
    (void)prefiltered;
    return guarded([&]() {
        check_params(P, D, M, features_dc, features_rest, scaling_raw, rotation_raw);
        R3_PARAMS_CALL();
        return forward_reserved({geom_buffer, binning_buffer, image_buffer}, reserve, c);
    });
}

static BwdCall backward_params_call(int P, const int* D, int M, int R, const float* background, int width, int height,
                                    const float* means3D, const float* features_dc, const float* features_rest,
                                    const float* scaling_raw, float scale_modifier, const float* rotation_raw,
                                    const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                                    float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                                    const float* dL_dpix, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity,
                                    float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dfeatures_dc,
                                    float* dL_dfeatures_rest, float* dL_dscaling_raw, float* dL_drotation_raw,
                                    float lambda_sh_sparsity, int debug, void* stream)
{
    check_params(P, D, M, features_dc, features_rest, scaling_raw, rotation_raw);
    if (P > 0 && (!dL_dfeatures_dc || (M > 1 && !dL_dfeatures_rest)))
        throw r3::Error("raw-parameter path: a gradient output pointer is NULL");
    return {P, D, M, R, background, width, height, means3D, features_dc, nullptr, scaling_raw, scale_modifier,
            rotation_raw, nullptr, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii,
            {geom_buffer, binning_buffer, image_buffer}, dL_dpix, dL_dmean2D, dL_dconic, dL_dopacity,
            dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dfeatures_dc, dL_dscaling_raw, dL_drotation_raw,
            lambda_sh_sparsity, debug, static_cast<hipStream_t>(stream), features_rest, dL_dfeatures_rest, 1};
}

int r3dgs_backward_params(int P, const int* D, int M, int R, const float* background, int width, int height,
                          const float* means3D, const float* features_dc, const float* features_rest, const float* scaling_raw,
                          float scale_modifier, const float* rotation_raw, const float* viewmatrix, const float* projmatrix,
                          const float* campos, float tan_fovx, float tan_fovy, const int* radii, char* geom_buffer,
                          char* binning_buffer, char* image_buffer, const float* dL_dpix, float* dL_dmean2D, float* dL_dconic,
                          float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dfeatures_dc,
                          float* dL_dfeatures_rest, float* dL_dscaling_raw, float* dL_drotation_raw, float lambda_sh_sparsity,
                          int debug, void* stream)
{
    return guarded([&]() {
        return backward_pass(backward_params_call(P, D, M, R, background, width, height, means3D, features_dc, features_rest,
                                                  scaling_raw, scale_modifier, rotation_raw, viewmatrix, projmatrix, campos,
                                                  tan_fovx, tan_fovy, radii, geom_buffer, binning_buffer, image_buffer, dL_dpix,
                                                  dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D,
                                                  dL_dfeatures_dc, dL_dfeatures_rest, dL_dscaling_raw, dL_drotation_raw,
                                                  lambda_sh_sparsity, debug, stream));
    });
}

int r3dgs_backward_params_absgrad(int P, const int* D, int M, int R, const float* background, int width, int height,
                                  const float* means3D, const float* features_dc, const float* features_rest,
                                  const float* scaling_raw, float scale_modifier, const float* rotation_raw,
                                  const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                                  float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                                  const float* dL_dpix, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                                  float* dL_dmean3D, float* dL_dcov3D, float* dL_dfeatures_dc, float* dL_dfeatures_rest,
                                  float* dL_dscaling_raw, float* dL_drotation_raw, float lambda_sh_sparsity, int debug,
                                  void* stream, float* dL_dmean2D_abs, float* abs_workspace, size_t abs_workspace_floats)
{
    return guarded([&]() {
        if (P > 0) check_absgrad_args(R, binning_buffer != nullptr, dL_dmean2D_abs, abs_workspace, abs_workspace_floats);
        BwdCall c = backward_params_call(P, D, M, R, background, width, height, means3D, features_dc, features_rest, scaling_raw,
                                         scale_modifier, rotation_raw, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii,
                                         geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_dmean2D, dL_dconic, dL_dopacity,
                                         dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dfeatures_dc, dL_dfeatures_rest, dL_dscaling_raw,
                                         dL_drotation_raw, lambda_sh_sparsity, debug, stream);
        ask_absgrad(c, dL_dmean2D_abs, abs_workspace, abs_workspace_floats);
        return backward_pass(c);
    });
}

int r3dgs_activate_params(int P, const float* scaling_raw, const float* rotation_raw, float* scales_out, float* rotations_out,
                          void* stream)
{
    return guarded([&]() {
        if (P <= 0) return 0;
        if ((scaling_raw == nullptr) != (scales_out == nullptr) || (rotation_raw == nullptr) != (rotations_out == nullptr))
            throw r3::Error("activate_params: an input without its output (or the reverse)");
        hipStream_t s = static_cast<hipStream_t>(stream);
        r3::launch_activate_params(P, scaling_raw, rotation_raw, scales_out, rotations_out, s);
        r3::check_launch("activate_params", s, false);
        return 0;
    });
}

// ---- the quantised model (include/r3dgs_quantised.h) -------------------------------------------------------------------
// The forward of r3dgs_inference_forward with the model read in place from codebook ids: the same plan, blobs, graph cache
// and reservation advice; only the two per-Gaussian stages have instantiations of their own (preprocess.hip).
#define R3_QUANT_CALL()                                                                                                 \
    const float *means3D = nullptr, *shs = nullptr, *colors_precomp = nullptr, *opacities = nullptr, *scales = nullptr,  \
                *rotations = nullptr, *cov3D_precomp = nullptr;                                                         \
    check_ragged(nullptr, bandsNum, coeffsNum, perBandPrimitiveCount, cumSumPrimitiveCount);                            \
    R3_FWD_CALL(coeffsNum, perBandPrimitiveCount, cumSumPrimitiveCount, 16);                                            \
    c.quantised = 1;                                                                                                    \
    c.quant.xyz = xyz;                                                                                                  \
    c.quant.xyz_is_half = xyz_is_half ? 1 : 0;                                                                          \
    c.quant.geom_ids = geom_ids;                                                                                        \
    c.quant.sh_ids = sh_ids;                                                                                            \
    c.quant.codebooks = codebooks

int r3dgs_quantised_forward(r3dgs_alloc_fn geometryBuffer, void* geometry_user, r3dgs_alloc_fn binningBuffer, void* binning_user,
                            r3dgs_alloc_fn imageBuffer, void* image_user, int P, const int* D, int bandsNum,
                            const int* coeffsNum, const int* perBandPrimitiveCount, const int* cumSumPrimitiveCount,
                            const float* background, int width, int height, const void* xyz, int xyz_is_half,
                            const unsigned char* geom_ids, const unsigned char* sh_ids, const float* codebooks,
                            float scale_modifier, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                            float tan_fovx, float tan_fovy, int prefiltered, float* out_color, int* out_touched_pixels,
                            float* out_transmittance, int* radii, int calculate_mean_transmittance, int debug, void* stream)
{
    (void)prefiltered;
    return guarded([&]() {
        R3_QUANT_CALL();
        return forward_exact({geometryBuffer, geometry_user, binningBuffer, binning_user, imageBuffer, image_user}, c);
    });
}

long long r3dgs_quantised_forward_reserved(char* geom_buffer, char* binning_buffer, char* image_buffer, int reserve, int P,
                                           const int* D, int bandsNum, const int* coeffsNum,
                                           const int* perBandPrimitiveCount, const int* cumSumPrimitiveCount,
                                           const float* background, int width, int height, const void* xyz, int xyz_is_half,
                                           const unsigned char* geom_ids, const unsigned char* sh_ids, const float* codebooks,
                                           float scale_modifier, const float* viewmatrix, const float* projmatrix,
                                           const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered,
                                           float* out_color, int* out_touched_pixels, float* out_transmittance, int* radii,
                                           int calculate_mean_transmittance, int debug, void* stream)
{
    (void)prefiltered;
    return guarded([&]() {
        R3_QUANT_CALL();
        return forward_reserved({geom_buffer, binning_buffer, image_buffer}, reserve, c);
    });
}

int r3dgs_quantised_decode(int P, const int* coeffsNum, const int* perBandPrimitiveCount, const int* cumSumPrimitiveCount,
                           const void* xyz, int xyz_is_half, const unsigned char* geom_ids, const unsigned char* sh_ids,
                           const float* codebooks, float* xyz_out, float* features_dc, float* features_rest, float* opacity,
                           float* scaling, float* rotation, int* degrees, void* stream)
{
    return guarded([&]() {
        if (P <= 0) return 0;
        if (!coeffsNum || !perBandPrimitiveCount || !cumSumPrimitiveCount || !xyz || !geom_ids || !sh_ids || !codebooks)
            throw r3::Error("quantised_decode: a required pointer is NULL");
        hipStream_t s = static_cast<hipStream_t>(stream);
        r3::QuantInputs q = {xyz, geom_ids, sh_ids, codebooks, xyz_is_half ? 1 : 0};
        r3::launch_quantised_decode(P, coeffsNum, perBandPrimitiveCount, cumSumPrimitiveCount, q, xyz_out, features_dc,
                                    features_rest, opacity, scaling, rotation, degrees, s);
        r3::check_launch("quantised_decode", s, false);
        return 0;
    });
}

size_t r3dgs_quantised_codebook_grad_workspace_bytes(int P) { return r3::quantised_codebook_grad_workspace_bytes(P); }

int r3dgs_quantised_codebook_grad(int P, const int* coeffsNum, const int* perBandPrimitiveCount, const int* cumSumPrimitiveCount,
                                  const unsigned char* geom_ids, const unsigned char* sh_ids, const float* dL_dfeatures_dc,
                                  const float* dL_dfeatures_rest, const float* dL_dopacity, const float* dL_dscaling,
                                  const float* dL_drotation, float* dL_dcodebooks, void* workspace, void* stream)
{
    return guarded([&]() {
        if (P < 0) throw r3::Error("quantised_codebook_grad: P < 0");
        if (!dL_dcodebooks) throw r3::Error("quantised_codebook_grad: dL_dcodebooks is NULL");
        if (P > 0 && (!coeffsNum || !perBandPrimitiveCount || !cumSumPrimitiveCount || !geom_ids || !sh_ids || !workspace))
            throw r3::Error("quantised_codebook_grad: a required pointer is NULL");
        hipStream_t s = static_cast<hipStream_t>(stream);
        r3::launch_quantised_codebook_grad(P, coeffsNum, perBandPrimitiveCount, cumSumPrimitiveCount, geom_ids, sh_ids,
                                           dL_dfeatures_dc, dL_dfeatures_rest, dL_dopacity, dL_dscaling, dL_drotation,
                                           dL_dcodebooks, workspace, s);
        r3::check_launch("quantised_codebook_grad", s, false);
        return 0;
    });
}

size_t r3dgs_quantised_bytes(int P, const int* perBandPrimitiveCount_host, int xyz_is_half)
{
    return guarded(
        [&]() {
            if (P < 0 || !perBandPrimitiveCount_host) throw r3::Error("quantised_bytes: P >= 0 and four per-degree counts");
            long long n = 0;
            for (int d = 0; d < 4; d++) {
                if (perBandPrimitiveCount_host[d] < 0) throw r3::Error("quantised_bytes: negative count");
                n += perBandPrimitiveCount_host[d];
            }
            if (n != P) throw r3::Error("quantised_bytes: the per-degree counts do not add up to P");
            return (size_t)r3::quant_model_bytes(P, perBandPrimitiveCount_host, xyz_is_half);
        },
        (size_t)0);
}

int r3dgs_colour_variance_accumulate(int P, const int* D, int M, int max_sh_deg, const float* means3D,
                                     const float* cam_pos, const float* shs, const int* radii,
                                     const int* touched_pixels, const float* transmittance, float* wSum, float* wSumSq,
                                     float* mean, float* variance, float* colourDistancesAccum, void* stream)
{
    return guarded([&]() {
        if (P <= 0) return 0;
        if (max_sh_deg < 1 || max_sh_deg > 3) throw r3::Error("max_sh_deg must be in [1,3]");
        if (M < (max_sh_deg + 1) * (max_sh_deg + 1) || M > 16) throw r3::Error("SH tensor too small for max_sh_deg");
        if (!D || !means3D || !cam_pos || !shs || !radii || !touched_pixels || !transmittance || !wSum || !wSumSq ||
            !mean || !variance || !colourDistancesAccum)
            throw r3::Error("a required pointer is NULL");
        hipStream_t s = static_cast<hipStream_t>(stream);
        r3::launch_colour_variance_accumulate(P, D, M, max_sh_deg, means3D, cam_pos, shs, radii, touched_pixels,
                                              transmittance, wSum, wSumSq, mean, variance, colourDistancesAccum, s);
        r3::check_launch("colour variance accumulate", s, false);
        return 0;
    });
}

int r3dgs_profile_enable(int on)
{
    profile_enable(on);
    return 0;
}

int r3dgs_profile_stage_count(void) { return kNumStages; }

const char* r3dgs_profile_stage_name(int stage)
{
    static const char* names[kNumStages] = {"preprocess_fwd", "depth_sort_scan", "tile_binning", "blend_fwd",
                                            "blend_bwd",      "preprocess_bwd",  "sh_color",        "blend_bwd_kernel"};
    return (stage >= 0 && stage < kNumStages) ? names[stage] : "";
}

int r3dgs_profile_read(double* total_ms, int* launches)
{
    return guarded([&]() {
        profile_read(total_ms, launches);
        return 0;
    });
}

int r3dgs_export_binning(int P, int R, int count, int width, int height, char* geom_buffer, char* binning_buffer,
                         char* image_buffer, uint64_t* keys, uint32_t* point_list, uint32_t* ranges, uint32_t* n_contrib,
                         float* final_T, uint32_t* tiles_touched, void* stream)
{
    return guarded([&]() {
        using namespace r3;
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (P <= 0) return 0;
        const TileGrid grid = grid_of(width, height);
        const size_t N = (size_t)width * height, Tn = grid.n();
        GeomState geom = GeomState::carve(geom_buffer, (size_t)P, cached_depth_temp((size_t)P));
        ImageState img = ImageState::carve(image_buffer, N, Tn);
        if (count > R) throw Error("count exceeds the blob's pair capacity");
        if (count > 0 && binning_buffer) {
            BinState bin = BinState::carve(binning_buffer, (size_t)R, pair_layout(P, Tn).wide, grid);
            if (keys) launch_export_keys(P, count, R, Tn, bin, geom, keys, s);
            if (point_list) {
                // entries beyond the pairs the pass binned (a caller holding only the reference's num_rendered may ask for
                // them: the exact-size blob is carved for that count) are not list entries: ~0, as the keys
                R3_HIP(hipMemsetAsync(point_list, 0xFF, sizeof(uint32_t) * (size_t)count, s));
                launch_export_point_list(count, bin.point_list, geom.header, point_list, s);
            }
        }
        if (ranges) R3_HIP(hipMemcpyAsync(ranges, img.ranges, sizeof(uint2) * Tn, hipMemcpyDeviceToDevice, s));
        if (n_contrib) R3_HIP(hipMemcpyAsync(n_contrib, img.n_contrib, sizeof(uint32_t) * N, hipMemcpyDeviceToDevice, s));
        if (final_T) R3_HIP(hipMemcpyAsync(final_T, img.final_T, sizeof(float) * N, hipMemcpyDeviceToDevice, s));
        if (tiles_touched)
            R3_HIP(hipMemcpyAsync(tiles_touched, geom.tiles, sizeof(uint32_t) * (size_t)P, hipMemcpyDeviceToDevice, s));
        check_launch("export", s, false);
        return 0;
    });
}

int r3dgs_export_tile_order(int P, int R, int width, int height, char* binning_buffer, char* image_buffer,
                            uint32_t* quad_depth, uint32_t* unit_order, void* stream)
{
    return guarded([&]() {
        using namespace r3;
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (!image_buffer) throw Error("a required pointer is NULL");
        const TileGrid grid = grid_of(width, height);
        const size_t Tn = grid.n();
        ImageState img = ImageState::carve(image_buffer, (size_t)width * height, Tn);
        if (quad_depth) R3_HIP(hipMemcpyAsync(quad_depth, img.quad_depth, sizeof(uint32_t) * 4 * Tn, hipMemcpyDeviceToDevice, s));
        if (unit_order) {
            if (!binning_buffer || R <= 0) throw Error("the unit order lives in the binning buffer");
            BinState bin = BinState::carve(binning_buffer, (size_t)R, pair_layout(P, Tn).wide, grid);
            R3_HIP(hipMemcpyAsync(unit_order, bin.unit_order, sizeof(uint32_t) * unit_order_words(bwd_units_cap((uint32_t)R, grid)),
                                  hipMemcpyDeviceToDevice, s));
        }
        check_launch("export", s, false);
        return 0;
    });
}

int r3dgs_bwd_units_cap(int R, int width, int height)
{
    return (int)bwd_units_cap((uint32_t)(R > 0 ? R : 1), grid_of(width, height));
}

}  // extern "C"
