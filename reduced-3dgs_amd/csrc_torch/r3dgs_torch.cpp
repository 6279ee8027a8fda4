// r3dgs_torch.cpp -- compiled torch binding of the rasterizer's hot calls (gfx950 / PyTorch-ROCm).
//
// The reference binds its rasterizer through a torch C++ extension (DGR/ext.cpp:16-25, rasterize_points.cu:136-305:
// tensors in, tensors out, resizable byte tensors behind the allocator callbacks).  This file is that layer for the MI355X
// library: a pybind module over the C ABI of include/r3dgs_rasterizer.h (libr3dgs_hip.so) -- it moves pointers, allocates
// the outputs and the three state blobs with at::empty on the current HIP stream's device, and calls the library.  There
// is no arithmetic here and no other path.  The module does not link against the library: _C.py hands it the addresses of
// the entry points of the libr3dgs_hip.so IT loaded (bind()), so both layers drive one library instance -- one graph
// cache, one reservation advisor -- whichever build R3DGS_LIB selected; an unbound module refuses every call.
//
// Scope: the two calls a training step makes -- the asynchronous forward (r3dgs_forward_reserved + the strict-mode check
// of the pass header) and the backward -- plus the fused training loss of r3dgs_loss.h (r3dgs_loss.py, r3dgs_exposure.py) and the fused Adam
// step of r3dgs_optim.h (r3dgs_optim.py).  Everything else (exact-size path, ragged inference forward, counter mode, the
// reduction operators, debug accessors) stays in the ctypes module diff_gaussian_rasterization/_C.py, which calls this
// one when it is built (R3DGS_BINDING=ctypes forces the pure-ctypes route).  Why it exists: at small scenes the step is
// host-bound and the ctypes marshalling of ~35 arguments per call is a third of it.
//
// Built by reduced-3dgs_amd/build.py with the host compiler against torch's headers (no hipify pass: the HIP-named c10
// headers are used directly).
#include <torch/extension.h>

// PyTorch-ROCm presents its HIP devices under the device type "cuda": the guard and stream accessors that accept that
// type are the *MasqueradingAsCUDA ones (the plain c10::hip::HIPGuard insists on DeviceType::HIP and throws)
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <limits>
#include <algorithm>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "r3dgs_aux.h"
#include "r3dgs_importance.h"
#include "r3dgs_loss.h"
#include "r3dgs_optim.h"
#include "r3dgs_quantised.h"
#include "r3dgs_rasterizer.h"
#include "r3dgs_trainstats.h"

namespace {

using at::Tensor;

// The entry points of the loaded libr3dgs_hip.so this module calls, once: X(name, required).  An optional one belongs to a
// family an older A/B build of the library lacks; its calls then refuse (need()).
#define R3_ENTRY_POINTS(X)                                    \
    X(r3dgs_last_error, true)                                 \
    X(r3dgs_version, true)                                    \
    X(r3dgs_geometry_bytes, true)                             \
    X(r3dgs_geometry_bytes_lean, true)                        \
    X(r3dgs_binning_bytes, true)                              \
    X(r3dgs_image_bytes, true)                                \
    X(r3dgs_forward_hint, true)                               \
    X(r3dgs_reserve_hint_view, true)                          \
    X(r3dgs_forward_reserved, true)                           \
    X(r3dgs_pass_query, true)                                 \
    X(r3dgs_backward, true)                                   \
    X(r3dgs_mark_visible, true)                               \
    X(r3dgs_aux_maps, true)                                   \
    X(r3dgs_aux_maps_backward_workspace_bytes, true)          \
    X(r3dgs_aux_maps_backward, true)                          \
    X(r3dgs_contribution_scores_workspace_bytes, true)        \
    X(r3dgs_contribution_scores, true)                        \
    X(r3dgs_l1_ssim_workspace_bytes, false)                   \
    X(r3dgs_l1_ssim_forward, false)                           \
    X(r3dgs_l1_ssim_backward, false)                          \
    X(r3dgs_l1_workspace_bytes, false)                        \
    X(r3dgs_l1_forward, false)                                \
    X(r3dgs_l1_backward, false)                               \
    X(r3dgs_adam_step, false)                                 \
    X(r3dgs_adam_step_capturable, false)                      \
    X(r3dgs_adam_step_visible, false)                         \
    X(r3dgs_adam_step_capturable_visible, false)              \
    X(r3dgs_forward_params, false)                            \
    X(r3dgs_forward_params_reserved, false)                   \
    X(r3dgs_backward_params, false)                           \
    X(r3dgs_activate_params, false)                           \
    X(r3dgs_train_stats_workspace_bytes, false)               \
    X(r3dgs_visible_means, false)                             \
    X(r3dgs_alpha_regul_backward, false)                      \
    X(r3dgs_densification_stats, false)                       \
    X(r3dgs_quantised_codebook_grad_workspace_bytes, false)   \
    X(r3dgs_quantised_codebook_grad, false)                   \
    X(r3dgs_absgrad_workspace_floats, false)                  \
    X(r3dgs_backward_absgrad, false)                          \
    X(r3dgs_backward_params_absgrad, false)                   \
    X(r3dgs_exposure_loss_workspace_bytes, false)             \
    X(r3dgs_exposure_loss_forward, false)                     \
    X(r3dgs_exposure_loss_backward, false)                    \
    X(r3dgs_exposure_apply, false)

struct Api {   // (types taken from the C headers)
#define R3_MEMBER(name, required) decltype(&::name) name = nullptr;
    R3_ENTRY_POINTS(R3_MEMBER)
#undef R3_MEMBER
    bool bound = false;
} api;

// what _C.py builds bind()'s address dict from: [(name, required)]
std::vector<std::pair<std::string, bool>> entry_points()
{
#define R3_LIST(name, required) {#name, required},
    return {R3_ENTRY_POINTS(R3_LIST)};
#undef R3_LIST
}

void bind(const std::map<std::string, uintptr_t>& addr)
{
#define R3_BIND(name, required)                                                                    \
    {                                                                                              \
        auto it = addr.find(#name);                                                                \
        const uintptr_t at = it == addr.end() ? 0 : it->second;                                    \
        if (required && !at) throw std::runtime_error("bind: no " #name);                          \
        api.name = reinterpret_cast<decltype(api.name)>(at);                                       \
    }
    R3_ENTRY_POINTS(R3_BIND)
#undef R3_BIND
    api.bound = true;
}

void need_bound()
{
    if (!api.bound) throw std::runtime_error("r3dgs torch binding: not bound to libr3dgs_hip.so (import diff_gaussian_rasterization._C)");
}

// an entry point of an optional family: `what` names the family the loaded library lacks
template <class Fn>
void need(Fn* entry, const char* what)
{
    need_bound();
    if (!entry) throw std::runtime_error(std::string("the loaded libr3dgs_hip.so has no ") + what + ": rebuild it with build.py");
}

[[noreturn]] void fail(const char* what)
{
    throw std::runtime_error(std::string(what) + ": " + api.r3dgs_last_error());
}

// absent optional input: an empty tensor, as the reference's wrapper passes torch.Tensor([])
// (diff_gaussian_rasterization/__init__.py:209-218)
template <class T>
const T* opt_ptr(const Tensor& t)
{
    return t.defined() && t.numel() != 0 ? t.data_ptr<T>() : nullptr;
}

// a state blob (or any byte buffer) as the C ABI takes it
char* blob_ptr(const Tensor& t) { return t.defined() && t.numel() != 0 ? reinterpret_cast<char*>(t.data_ptr()) : nullptr; }

// an input as the library reads it: on `dev`, of `type`, contiguous (copied if it is not); undefined for an absent one
Tensor dev_as(const Tensor& t, const c10::Device& dev, at::ScalarType type, const char* type_name)
{
    if (!t.defined() || t.numel() == 0) return Tensor();
    if (t.device() != dev) throw std::runtime_error("expected a tensor on " + dev.str() + ", got " + t.device().str());
    if (t.scalar_type() != type) throw std::runtime_error(std::string("expected ") + type_name + ", got " + c10::toString(t.scalar_type()));
    return t.contiguous();
}
Tensor dev_f32(const Tensor& t, const c10::Device& dev) { return dev_as(t, dev, at::kFloat, "float32"); }
Tensor dev_i32(const Tensor& t, const c10::Device& dev) { return dev_as(t, dev, at::kInt, "int32"); }

// a backward's result for P == 0: zeros of the given shapes
std::vector<Tensor> zero_grads(const at::TensorOptions& f32, std::initializer_list<std::vector<int64_t>> shapes)
{
    std::vector<Tensor> out;
    for (const std::vector<int64_t>& shape : shapes) out.push_back(at::zeros(shape, f32));
    return out;
}

void* cur_stream(const c10::Device& dev) { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream(); }

std::mutex g_mu;
std::map<std::tuple<int, int, int, int, int>, size_t> g_sizes;   // (kind, a, b, c, d) -> bytes

size_t blob_bytes(int kind, int a, int b = 0, int c = 0, int d = 0)
{
    std::lock_guard<std::mutex> lk(g_mu);
    const auto key = std::make_tuple(kind, a, b, c, d);
    auto it = g_sizes.find(key);
    if (it != g_sizes.end()) return it->second;
    size_t v = 0;
    switch (kind) {
        case 0: v = api.r3dgs_geometry_bytes(a); break;
        case 1: v = api.r3dgs_geometry_bytes_lean(a); break;
        case 2: v = api.r3dgs_binning_bytes(a, b, c, d); break;
        default: v = api.r3dgs_image_bytes(a, b); break;
    }
    if (v == 0) fail("rasterize_gaussians");
    if (g_sizes.size() > 4096) g_sizes.clear();
    g_sizes[key] = v;
    return v;
}

using ReservedPass = std::tuple<long long, int, int, int, Tensor, Tensor, Tensor, Tensor, Tensor>;

// What the reserved forwards share behind their argument checks (the caller holds the device guard): the hint, the pair
// reservation (`reserve_override` > 0: a chosen one), out_color / radii and the three blobs, the entry point --
// call(geom, binning, img, reserve, out_color, radii, stream) -> ticket -- and, when `strict`, the wait for the pass's HEADER
// (not for the pass) with the GIL released.  `what` names the caller in errors.
// -> (ticket, reserve, num_rendered, flags, out_color, radii, geom, binning, img).  ticket == 0: nothing is known about this
// view size yet -- the caller takes the exact-size path.  num_rendered / flags are filled (>= 0) when `strict`.
template <class Call>
ReservedPass reserved_pass(const char* what, const c10::Device& dev, int P, int W, int H, const Tensor& vm, bool trains, bool lean,
                           bool strict, int64_t reserve_override, Call&& call)
{
    api.r3dgs_forward_hint(trains ? 1 : 0);
    const int reserve = reserve_override > 0 ? (int)reserve_override : api.r3dgs_reserve_hint_view(P, W, H, opt_ptr<float>(vm));
    if (reserve < 0) fail(what);
    Tensor none;
    if (reserve == 0 || P == 0) return {0LL, 0, -1, 0, none, none, none, none, none};
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev), i32 = f32.dtype(at::kInt), u8 = f32.dtype(at::kByte);
    Tensor out_color = at::empty({3, H, W}, f32), radii = at::empty({P}, i32);
    Tensor geom = at::empty({(int64_t)blob_bytes(lean ? 1 : 0, P)}, u8);
    Tensor binning = at::empty({(int64_t)blob_bytes(2, P, W, H, reserve)}, u8);
    Tensor img = at::empty({(int64_t)blob_bytes(3, W, H)}, u8);
    const long long ticket = call(reinterpret_cast<char*>(geom.data_ptr()), reinterpret_cast<char*>(binning.data_ptr()),
                                  reinterpret_cast<char*>(img.data_ptr()), reserve, out_color.data_ptr<float>(),
                                  radii.data_ptr<int>(), cur_stream(dev));
    if (ticket < 0) fail(what);
    int rendered = -1, flags = 0;
    if (strict && ticket > 0) {
        int visible = 0, cap = 0, st;
        {
            pybind11::gil_scoped_release nogil;   // a poll of host memory with short sleeps inside the library
            st = api.r3dgs_pass_query(ticket, 1, &rendered, &visible, &cap, &flags);
        }
        if (st < 0) fail("num_rendered");
        if (st != 1) rendered = -1;
    }
    return {ticket, reserve, rendered, flags, out_color, radii, geom, binning, img};
}

// RasterizeGaussiansCUDA (rasterize_points.cu:136-222) on the asynchronous path -> as reserved_pass
ReservedPass forward_reserved(
    const Tensor& background, const Tensor& means3D, const Tensor& colors, const Tensor& opacity, const Tensor& scales,
    const Tensor& rotations, double scale_modifier, const Tensor& cov3D_precomp, const Tensor& viewmatrix,
    const Tensor& projmatrix, double tan_fovx, double tan_fovy, int64_t image_height, int64_t image_width, const Tensor& sh,
    const Tensor& degrees, const Tensor& campos, bool prefiltered, bool trains, bool strict)
{
    need_bound();
    if (means3D.dim() != 2 || means3D.size(1) != 3)
        throw std::runtime_error("means3D must have dimensions (num_points, 3)");   // rasterize_points.cu:158-161
    const c10::Device dev = means3D.device();
    if (!dev.is_cuda()) throw std::runtime_error("the MI355X rasterizer needs device tensors (no CPU path)");
    const int P = (int)means3D.size(0), H = (int)image_height, W = (int)image_width;
    const Tensor bg = dev_f32(background, dev), m3 = dev_f32(means3D, dev), col = dev_f32(colors, dev);
    const Tensor op = dev_f32(opacity, dev), sc = dev_f32(scales, dev), rot = dev_f32(rotations, dev);
    const Tensor cov = dev_f32(cov3D_precomp, dev), vm = dev_f32(viewmatrix, dev), pm = dev_f32(projmatrix, dev);
    const Tensor cp = dev_f32(campos, dev), shc = dev_f32(sh, dev), deg = dev_i32(degrees, dev);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const bool lean = !trains || !shc.defined() || col.defined();   // no SH direction derivatives will be left
    const int M = shc.defined() ? (int)shc.size(1) : 0;
    return reserved_pass("rasterize_gaussians", dev, P, W, H, vm, trains, lean, strict, 0,
                         [&](char* geom, char* binning, char* img, int reserve, float* out_color, int* radii, void* stream) {
        return api.r3dgs_forward_reserved(
            geom, binning, img, reserve, P, opt_ptr<int>(deg), M, opt_ptr<float>(bg), W, H, opt_ptr<float>(m3), opt_ptr<float>(shc),
            opt_ptr<float>(col), opt_ptr<float>(op), opt_ptr<float>(sc), (float)scale_modifier, opt_ptr<float>(rot),
            opt_ptr<float>(cov), opt_ptr<float>(vm), opt_ptr<float>(pm), opt_ptr<float>(cp), (float)tan_fovx, (float)tan_fovy,
            prefiltered ? 1 : 0, out_color, nullptr, nullptr, radii, 0, 0, stream);
    });
}

// RasterizeGaussiansBackwardCUDA (rasterize_points.cu:224-305).  `capacity`: the pair capacity the forward carved the
// binning blob with.  Every element of every output is written by the library: at::empty, no fills.
// absgrad: through r3dgs_backward_absgrad, + dL_dmeans2D_abs [P,3] as the last element (the workspace is this call's own).
std::vector<Tensor> backward_impl(const Tensor& background, const Tensor& means3D, const Tensor& radii, const Tensor& colors,
                                  const Tensor& scales, const Tensor& rotations, double scale_modifier, const Tensor& cov3D_precomp,
                                  const Tensor& viewmatrix, const Tensor& projmatrix, double tan_fovx, double tan_fovy,
                                  const Tensor& dL_dout_color, const Tensor& sh, const Tensor& degrees, const Tensor& campos,
                                  const Tensor& geomBuffer, int64_t capacity, const Tensor& binningBuffer, const Tensor& imageBuffer,
                                  double lambda_sh_sparsity, bool debug, bool want_conic, bool absgrad)
{
    need_bound();
    if (absgrad) {
        need(api.r3dgs_backward_absgrad, "absolute-gradient entry points (r3dgs_backward_absgrad)");
        need(api.r3dgs_absgrad_workspace_floats, "absolute-gradient entry points (r3dgs_backward_absgrad)");
    }
    const c10::Device dev = means3D.device();
    const int P = (int)means3D.size(0);
    const int H = (int)dL_dout_color.size(1), W = (int)dL_dout_color.size(2);
    const int M = (sh.defined() && sh.numel() != 0) ? (int)sh.size(1) : 0;
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
    if (P == 0) {
        std::vector<Tensor> z = zero_grads(f32, {{0, 3}, {0, 3}, {0, 1}, {0, 3}, {0, 6}, {0, M, 3}, {0, 3}, {0, 4}});
        if (absgrad) z.push_back(at::zeros({0, 3}, f32));
        return z;
    }
    Tensor dL_dmeans3D = at::empty({P, 3}, f32), dL_dmeans2D = at::empty({P, 3}, f32), dL_dcolors = at::empty({P, 3}, f32);
    Tensor dL_dopacity = at::empty({P, 1}, f32), dL_dcov3D = at::empty({P, 6}, f32), dL_dsh = at::empty({P, M, 3}, f32);
    Tensor dL_dscales = at::empty({P, 3}, f32), dL_drotations = at::empty({P, 4}, f32);
    Tensor dL_dconic = want_conic ? at::empty({P, 2, 2}, f32) : Tensor();
    const Tensor bg = dev_f32(background, dev), m3 = dev_f32(means3D, dev), col = dev_f32(colors, dev);
    const Tensor sc = dev_f32(scales, dev), rot = dev_f32(rotations, dev), cov = dev_f32(cov3D_precomp, dev);
    const Tensor vm = dev_f32(viewmatrix, dev), pm = dev_f32(projmatrix, dev), cp = dev_f32(campos, dev);
    const Tensor g = dev_f32(dL_dout_color, dev), shc = dev_f32(sh, dev), deg = dev_i32(degrees, dev), rad = dev_i32(radii, dev);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    Tensor dL_abs, abs_ws;
    if (absgrad) {
        dL_abs = at::empty({P, 3}, f32);
        abs_ws = at::empty({(int64_t)api.r3dgs_absgrad_workspace_floats((int)capacity)}, f32);
    }
#define R3_BACKWARD_ARGS                                                                                                  \
    P, opt_ptr<int>(deg), M, (int)capacity, opt_ptr<float>(bg), W, H, opt_ptr<float>(m3), opt_ptr<float>(shc),            \
        opt_ptr<float>(col), opt_ptr<float>(sc), (float)scale_modifier, opt_ptr<float>(rot), opt_ptr<float>(cov),         \
        opt_ptr<float>(vm), opt_ptr<float>(pm), opt_ptr<float>(cp), (float)tan_fovx, (float)tan_fovy, opt_ptr<int>(rad),  \
        blob_ptr(geomBuffer), blob_ptr(binningBuffer), blob_ptr(imageBuffer), opt_ptr<float>(g),                          \
        dL_dmeans2D.data_ptr<float>(), dL_dconic.defined() ? dL_dconic.data_ptr<float>() : nullptr,                       \
        dL_dopacity.data_ptr<float>(), dL_dcolors.data_ptr<float>(), dL_dmeans3D.data_ptr<float>(),                       \
        dL_dcov3D.data_ptr<float>(), M ? dL_dsh.data_ptr<float>() : nullptr, dL_dscales.data_ptr<float>(),                \
        dL_drotations.data_ptr<float>(), (float)lambda_sh_sparsity, debug ? 1 : 0, cur_stream(dev)
    const int st = absgrad ? api.r3dgs_backward_absgrad(R3_BACKWARD_ARGS, dL_abs.data_ptr<float>(), abs_ws.data_ptr<float>(),
                                                        (size_t)abs_ws.numel())
                           : api.r3dgs_backward(R3_BACKWARD_ARGS);
#undef R3_BACKWARD_ARGS
    if (st < 0) fail("rasterize_gaussians_backward");
    std::vector<Tensor> out{dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations};
    if (want_conic) out.push_back(dL_dconic);
    if (absgrad) out.push_back(dL_abs);
    return out;
}

#define R3_BACKWARD_PARAMS                                                                                                     \
    const Tensor &background, const Tensor &means3D, const Tensor &radii, const Tensor &colors, const Tensor &scales,          \
        const Tensor &rotations, double scale_modifier, const Tensor &cov3D_precomp, const Tensor &viewmatrix,                 \
        const Tensor &projmatrix, double tan_fovx, double tan_fovy, const Tensor &dL_dout_color, const Tensor &sh,             \
        const Tensor &degrees, const Tensor &campos, const Tensor &geomBuffer, int64_t capacity, const Tensor &binningBuffer,  \
        const Tensor &imageBuffer, double lambda_sh_sparsity, bool debug, bool want_conic
#define R3_BACKWARD_PASS                                                                                                       \
    background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,    \
        tan_fovy, dL_dout_color, sh, degrees, campos, geomBuffer, capacity, binningBuffer, imageBuffer, lambda_sh_sparsity,    \
        debug, want_conic
std::vector<Tensor> backward(R3_BACKWARD_PARAMS) { return backward_impl(R3_BACKWARD_PASS, false); }
std::vector<Tensor> backward_absgrad(R3_BACKWARD_PARAMS) { return backward_impl(R3_BACKWARD_PASS, true); }
#undef R3_BACKWARD_PARAMS
#undef R3_BACKWARD_PASS

// ---- raster from the model's raw parameters (r3dgs_*_params): the same marshalling as diff_gaussian_rasterization/_C.py's
// rasterize_gaussian_params*; refusals (shapes, dtypes, contiguity) carry the same messages.

void need_params() { need(api.r3dgs_forward_params_reserved, "raw-parameter entry points"); }

// a raw parameter tensor: on `dev`, fp32, contiguous AS PASSED (a copy would defeat the point of the path)
const float* param_ptr(const Tensor& t, const c10::Device& dev, const char* name)
{
    if (t.device() != dev) throw std::runtime_error(std::string(name) + ": expected a tensor on " + dev.str() + ", got " + t.device().str());
    if (t.scalar_type() != at::kFloat)
        throw std::runtime_error(std::string(name) + ": the raw-parameter path needs float32, got " + c10::toString(t.scalar_type()));
    if (!t.is_contiguous()) throw std::runtime_error(std::string(name) + ": the raw-parameter path needs a contiguous tensor");
    return t.numel() ? t.data_ptr<float>() : nullptr;
}

struct ParamPtrs {
    int P, M;
    const float *xyz, *dc, *rest, *opacity, *scaling, *rotation;
};

ParamPtrs check_params(const Tensor& xyz, const Tensor& features_dc, const Tensor& features_rest, const Tensor& opacity,
                       const Tensor& scaling, const Tensor& rotation, const Tensor& degrees)
{
    if (xyz.dim() != 2 || xyz.size(1) != 3) throw std::runtime_error("means3D must have dimensions (num_points, 3)");
    const c10::Device dev = xyz.device();
    if (!dev.is_cuda()) throw std::runtime_error("the MI355X rasterizer needs device tensors (no CPU path)");
    ParamPtrs p;
    p.P = (int)xyz.size(0);
    if (features_dc.dim() != 3 || features_dc.size(0) != p.P || features_dc.size(1) != 1 || features_dc.size(2) != 3)
        throw std::runtime_error("features_dc must have dimensions (num_points, 1, 3)");
    const bool no_rest = !features_rest.defined() || features_rest.numel() == 0;
    if (!no_rest && (features_rest.dim() != 3 || features_rest.size(0) != p.P || features_rest.size(2) != 3))
        throw std::runtime_error("features_rest must have dimensions (num_points, M-1, 3)");
    p.M = no_rest ? 1 : 1 + (int)features_rest.size(1);
    if (p.M > 16) throw std::runtime_error("features_rest must have dimensions (num_points, M-1, 3) with M <= 16");
    if (scaling.dim() != 2 || scaling.size(0) != p.P || scaling.size(1) != 3)
        throw std::runtime_error("scaling must have dimensions (num_points, 3)");
    if (rotation.dim() != 2 || rotation.size(0) != p.P || rotation.size(1) != 4)
        throw std::runtime_error("rotation must have dimensions (num_points, 4)");
    if (opacity.numel() != p.P) throw std::runtime_error("opacity must have dimensions (num_points, 1)");
    if (degrees.numel() != p.P) throw std::runtime_error("degrees must have one entry per point");
    p.xyz = param_ptr(xyz, dev, "means3D");
    p.dc = param_ptr(features_dc, dev, "features_dc");
    p.rest = no_rest ? nullptr : param_ptr(features_rest, dev, "features_rest");
    p.opacity = param_ptr(opacity, dev, "opacity");
    p.scaling = param_ptr(scaling, dev, "scaling");
    p.rotation = param_ptr(rotation, dev, "rotation");
    return p;
}

// -> as reserved_pass
ReservedPass forward_params_reserved(
    const Tensor& background, const Tensor& xyz, const Tensor& features_dc, const Tensor& features_rest, const Tensor& degrees,
    const Tensor& opacity, const Tensor& scaling, const Tensor& rotation, double scale_modifier, const Tensor& viewmatrix,
    const Tensor& projmatrix, double tan_fovx, double tan_fovy, int64_t image_height, int64_t image_width, const Tensor& campos,
    bool prefiltered, bool trains, bool strict, int64_t reserve_override)
{
    need_params();
    const ParamPtrs p = check_params(xyz, features_dc, features_rest, opacity, scaling, rotation, degrees);
    const c10::Device dev = xyz.device();
    const int P = p.P, H = (int)image_height, W = (int)image_width;
    const Tensor bg = dev_f32(background, dev), vm = dev_f32(viewmatrix, dev), pm = dev_f32(projmatrix, dev);
    const Tensor cp = dev_f32(campos, dev), deg = dev_i32(degrees, dev);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    return reserved_pass("rasterize_gaussian_params", dev, P, W, H, vm, trains, !trains, strict, reserve_override,
                         [&](char* geom, char* binning, char* img, int reserve, float* out_color, int* radii, void* stream) {
        return api.r3dgs_forward_params_reserved(
            geom, binning, img, reserve, P, opt_ptr<int>(deg), p.M, opt_ptr<float>(bg), W, H, p.xyz, p.dc, p.rest, p.opacity,
            p.scaling, (float)scale_modifier, p.rotation, opt_ptr<float>(vm), opt_ptr<float>(pm), opt_ptr<float>(cp),
            (float)tan_fovx, (float)tan_fovy, prefiltered ? 1 : 0, out_color, nullptr, nullptr, radii, 0, 0, stream);
    });
}

// the exact-size path (r3dgs_forward_params): the three blobs are byte tensors allocated from the library's callbacks
struct BlobSlot {
    Tensor t;
    c10::Device dev;
    bool failed = false;
    explicit BlobSlot(c10::Device d) : dev(d) {}
};
char* blob_alloc(size_t bytes, void* user)
{
    BlobSlot* b = static_cast<BlobSlot*>(user);
    try {
        b->t = at::empty({(int64_t)bytes}, at::TensorOptions().dtype(at::kByte).device(b->dev));
        return reinterpret_cast<char*>(b->t.data_ptr());
    } catch (...) {   // an exception cannot cross the C frame
        b->failed = true;
        return nullptr;
    }
}

// -> (num_rendered, out_color, radii, geom, binning, img)
std::tuple<int, Tensor, Tensor, Tensor, Tensor, Tensor> forward_params(
    const Tensor& background, const Tensor& xyz, const Tensor& features_dc, const Tensor& features_rest, const Tensor& degrees,
    const Tensor& opacity, const Tensor& scaling, const Tensor& rotation, double scale_modifier, const Tensor& viewmatrix,
    const Tensor& projmatrix, double tan_fovx, double tan_fovy, int64_t image_height, int64_t image_width, const Tensor& campos,
    bool prefiltered, bool trains, bool debug)
{
    need_params();
    const ParamPtrs p = check_params(xyz, features_dc, features_rest, opacity, scaling, rotation, degrees);
    const c10::Device dev = xyz.device();
    const int P = p.P, H = (int)image_height, W = (int)image_width;
    const Tensor bg = dev_f32(background, dev), vm = dev_f32(viewmatrix, dev), pm = dev_f32(projmatrix, dev);
    const Tensor cp = dev_f32(campos, dev), deg = dev_i32(degrees, dev);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev), i32 = f32.dtype(at::kInt);
    Tensor out_color = at::empty({3, H, W}, f32), radii = at::empty({P}, i32);
    BlobSlot geom(dev), binning(dev), img(dev);
    api.r3dgs_forward_hint(trains ? 1 : 0);
    const int rendered = api.r3dgs_forward_params(
        blob_alloc, &geom, blob_alloc, &binning, blob_alloc, &img, P, opt_ptr<int>(deg), p.M, opt_ptr<float>(bg), W, H, p.xyz, p.dc,
        p.rest, p.opacity, p.scaling, (float)scale_modifier, p.rotation, opt_ptr<float>(vm), opt_ptr<float>(pm),
        opt_ptr<float>(cp), (float)tan_fovx, (float)tan_fovy, prefiltered ? 1 : 0, out_color.data_ptr<float>(), nullptr, nullptr,
        radii.data_ptr<int>(), 0, debug ? 1 : 0, cur_stream(dev));
    if (geom.failed || binning.failed || img.failed) throw std::runtime_error("rasterize_gaussian_params: a state buffer could not be allocated");
    if (rendered < 0) fail("rasterize_gaussian_params");
    const auto u8 = f32.dtype(at::kByte);
    auto blob = [&](BlobSlot& b) { return b.t.defined() ? b.t : at::empty({0}, u8); };
    return {rendered, out_color, radii, blob(geom), blob(binning), blob(img)};
}

// -> (dL_dmeans2D, dL_dopacity, dL_dmeans3D, dL_dfeatures_dc, dL_dfeatures_rest, dL_dscaling, dL_drotation): gradients of
// the tensors passed in, each written whole by the library into at::empty storage of the leaf's own shape
// absgrad: through r3dgs_backward_params_absgrad, + dL_dmeans2D_abs [P,3] as the last element
std::vector<Tensor> backward_params_impl(const Tensor& background, const Tensor& xyz, const Tensor& radii, const Tensor& features_dc,
                                         const Tensor& features_rest, const Tensor& degrees, const Tensor& opacity,
                                         const Tensor& scaling, const Tensor& rotation, double scale_modifier,
                                         const Tensor& viewmatrix, const Tensor& projmatrix, double tan_fovx, double tan_fovy,
                                         const Tensor& dL_dout_color, const Tensor& campos, const Tensor& geomBuffer,
                                         int64_t capacity, const Tensor& binningBuffer, const Tensor& imageBuffer,
                                         double lambda_sh_sparsity, bool debug, bool absgrad)
{
    need_params();
    if (absgrad) {
        need(api.r3dgs_backward_params_absgrad, "absolute-gradient entry points (r3dgs_backward_absgrad)");
        need(api.r3dgs_absgrad_workspace_floats, "absolute-gradient entry points (r3dgs_backward_absgrad)");
    }
    const ParamPtrs p = check_params(xyz, features_dc, features_rest, opacity, scaling, rotation, degrees);
    const c10::Device dev = xyz.device();
    const int P = p.P, M = p.M;
    const int H = (int)dL_dout_color.size(1), W = (int)dL_dout_color.size(2);
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
    if (P == 0) {
        std::vector<Tensor> z = zero_grads(f32, {{0, 3}, {0, 1}, {0, 3}, {0, 1, 3}, {0, M - 1, 3}, {0, 3}, {0, 4}});
        if (absgrad) z.push_back(at::zeros({0, 3}, f32));
        return z;
    }
    Tensor dL_dmeans3D = at::empty({P, 3}, f32), dL_dmeans2D = at::empty({P, 3}, f32), dL_dopacity = at::empty({P, 1}, f32);
    Tensor dL_ddc = at::empty({P, 1, 3}, f32), dL_drest = at::empty({P, M - 1, 3}, f32);
    Tensor dL_dscaling = at::empty({P, 3}, f32), dL_drotation = at::empty({P, 4}, f32);
    // what the C ABI also writes and this path has no leaf for (precomputed colours / covariances): one scratch tensor
    Tensor scratch = at::empty({P, 9}, f32);
    const Tensor bg = dev_f32(background, dev), vm = dev_f32(viewmatrix, dev), pm = dev_f32(projmatrix, dev);
    const Tensor cp = dev_f32(campos, dev), g = dev_f32(dL_dout_color, dev), deg = dev_i32(degrees, dev), rad = dev_i32(radii, dev);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    Tensor dL_abs, abs_ws;
    if (absgrad) {
        dL_abs = at::empty({P, 3}, f32);
        abs_ws = at::empty({(int64_t)api.r3dgs_absgrad_workspace_floats((int)capacity)}, f32);
    }
#define R3_BACKWARD_ARGS                                                                                                      \
    P, opt_ptr<int>(deg), M, (int)capacity, opt_ptr<float>(bg), W, H, p.xyz, p.dc, p.rest, p.scaling, (float)scale_modifier,  \
        p.rotation, opt_ptr<float>(vm), opt_ptr<float>(pm), opt_ptr<float>(cp), (float)tan_fovx, (float)tan_fovy,             \
        opt_ptr<int>(rad), blob_ptr(geomBuffer), blob_ptr(binningBuffer), blob_ptr(imageBuffer), opt_ptr<float>(g),           \
        dL_dmeans2D.data_ptr<float>(), nullptr, dL_dopacity.data_ptr<float>(), scratch.data_ptr<float>(),                     \
        dL_dmeans3D.data_ptr<float>(), scratch.data_ptr<float>() + 3 * (size_t)P, dL_ddc.data_ptr<float>(),                   \
        M > 1 ? dL_drest.data_ptr<float>() : nullptr, dL_dscaling.data_ptr<float>(), dL_drotation.data_ptr<float>(),          \
        (float)lambda_sh_sparsity, debug ? 1 : 0, cur_stream(dev)
    const int st = absgrad ? api.r3dgs_backward_params_absgrad(R3_BACKWARD_ARGS, dL_abs.data_ptr<float>(),
                                                               abs_ws.data_ptr<float>(), (size_t)abs_ws.numel())
                           : api.r3dgs_backward_params(R3_BACKWARD_ARGS);
#undef R3_BACKWARD_ARGS
    if (st < 0) fail("rasterize_gaussian_params_backward");
    std::vector<Tensor> out{dL_dmeans2D, dL_dopacity, dL_dmeans3D, dL_ddc, dL_drest, dL_dscaling, dL_drotation};
    if (absgrad) out.push_back(dL_abs);
    return out;
}

#define R3_BACKWARD_PARAMS                                                                                                     \
    const Tensor &background, const Tensor &xyz, const Tensor &radii, const Tensor &features_dc, const Tensor &features_rest,  \
        const Tensor &degrees, const Tensor &opacity, const Tensor &scaling, const Tensor &rotation, double scale_modifier,    \
        const Tensor &viewmatrix, const Tensor &projmatrix, double tan_fovx, double tan_fovy, const Tensor &dL_dout_color,     \
        const Tensor &campos, const Tensor &geomBuffer, int64_t capacity, const Tensor &binningBuffer,                         \
        const Tensor &imageBuffer, double lambda_sh_sparsity, bool debug
#define R3_BACKWARD_PASS                                                                                                       \
    background, xyz, radii, features_dc, features_rest, degrees, opacity, scaling, rotation, scale_modifier, viewmatrix,       \
        projmatrix, tan_fovx, tan_fovy, dL_dout_color, campos, geomBuffer, capacity, binningBuffer, imageBuffer,               \
        lambda_sh_sparsity, debug
std::vector<Tensor> backward_params(R3_BACKWARD_PARAMS) { return backward_params_impl(R3_BACKWARD_PASS, false); }
std::vector<Tensor> backward_params_absgrad(R3_BACKWARD_PARAMS) { return backward_params_impl(R3_BACKWARD_PASS, true); }
#undef R3_BACKWARD_PARAMS
#undef R3_BACKWARD_PASS

// r3dgs_aux_maps over the three buffers a forward returned -> (depth, alpha, median_depth [1,H,W], T_check [H,W],
// n_check int32 [H,W]); a map that was not asked for is an undefined tensor.  `capacity`: as backward's.
std::vector<Tensor> aux_maps(int64_t P, int64_t capacity, int64_t image_height, int64_t image_width, const Tensor& geomBuffer,
                             const Tensor& binningBuffer, const Tensor& imageBuffer, bool want_depth, bool want_alpha,
                             bool want_median, bool want_checks)
{
    need_bound();
    c10::Device dev = imageBuffer.defined() && imageBuffer.numel() ? imageBuffer.device() : geomBuffer.device();
    if (P != 0) {
        if (!dev.is_cuda()) throw std::runtime_error("the MI355X rasterizer needs device tensors (no CPU path)");
        if (geomBuffer.device() != dev || binningBuffer.device() != dev || imageBuffer.device() != dev)
            throw std::runtime_error("aux_maps: the three state buffers must live on one device");
    } else if (!dev.is_cuda()) {   // nothing says where: the current device, as the forward's empty result
        dev = c10::Device(c10::DeviceType::CUDA, c10::hip::current_device());
    }
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
    const int H = (int)image_height, W = (int)image_width;
    Tensor depth, alpha, median, T_check, n_check;
    if (want_depth) depth = at::empty({1, H, W}, f32);
    if (want_alpha) alpha = at::empty({1, H, W}, f32);
    if (want_median) median = at::empty({1, H, W}, f32);
    if (want_checks) {
        T_check = at::empty({H, W}, f32);
        n_check = at::empty({H, W}, f32.dtype(at::kInt));
    }
    auto fp = [](const Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; };
    if (api.r3dgs_aux_maps((int)P, (int)capacity, W, H, blob_ptr(geomBuffer), blob_ptr(binningBuffer), blob_ptr(imageBuffer),
                           fp(depth), fp(alpha), fp(median), fp(T_check),
                           n_check.defined() ? reinterpret_cast<unsigned*>(n_check.data_ptr<int>()) : nullptr, cur_stream(dev)) < 0)
        fail("aux_maps");
    return {depth, alpha, median, T_check, n_check};
}

// r3dgs_contribution_scores over the three buffers a forward returned, into the caller's [P] tensors in place (an empty
// tensor: not computed; _C.py has checked devices, dtypes, sizes and contiguity: nothing is copied) -> (T_check [H,W],
// n_check int32 [H,W]), undefined unless asked for.  `capacity`: as backward's.
std::vector<Tensor> contribution_scores(int64_t P, int64_t capacity, int64_t image_height, int64_t image_width,
                                        const Tensor& geomBuffer, const Tensor& binningBuffer, const Tensor& imageBuffer,
                                        const Tensor& pixel_weight, const Tensor& score_sum, const Tensor& score_max,
                                        const Tensor& score_count, const Tensor& score_views, bool accumulate, bool want_checks)
{
    need_bound();
    c10::Device dev = imageBuffer.defined() && imageBuffer.numel() ? imageBuffer.device() : geomBuffer.device();
    if (P != 0) {
        if (!dev.is_cuda()) throw std::runtime_error("the MI355X rasterizer needs device tensors (no CPU path)");
    } else if (!dev.is_cuda()) {   // nothing says where: the current device, as the forward's empty result
        dev = c10::Device(c10::DeviceType::CUDA, c10::hip::current_device());
    }
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
    const int H = (int)image_height, W = (int)image_width;
    Tensor T_check, n_check;
    if (want_checks) {
        T_check = at::empty({H, W}, f32);
        n_check = at::empty({H, W}, f32.dtype(at::kInt));
    }
    const size_t nbytes = api.r3dgs_contribution_scores_workspace_bytes((int)P, (int)capacity, W, H);
    if (nbytes == 0 && P != 0 && capacity != 0) fail("contribution_scores_workspace_bytes");
    const Tensor work = at::empty({(int64_t)std::max<size_t>(nbytes, 1)}, f32.dtype(at::kByte));
    auto ptr = [](const Tensor& t) { return t.defined() && t.numel() != 0 ? t.data_ptr() : nullptr; };
    if (api.r3dgs_contribution_scores((int)P, (int)capacity, W, H, blob_ptr(geomBuffer), blob_ptr(binningBuffer),
                                      blob_ptr(imageBuffer), static_cast<const float*>(ptr(pixel_weight)),
                                      static_cast<double*>(ptr(score_sum)), static_cast<float*>(ptr(score_max)),
                                      static_cast<long long*>(ptr(score_count)), static_cast<int*>(ptr(score_views)),
                                      accumulate ? 1 : 0, static_cast<float*>(ptr(T_check)), static_cast<unsigned*>(ptr(n_check)),
                                      blob_ptr(work), cur_stream(dev)) < 0)
        fail("contribution_scores");
    return {T_check, n_check};
}

// -> (scales [P,3], rotations [P,4]) by csrc/param_math.h, the values the raw-parameter kernels use
std::tuple<Tensor, Tensor> activate_params(const Tensor& scaling, const Tensor& rotation)
{
    need_params();
    const c10::Device dev = scaling.device();
    if (!dev.is_cuda()) throw std::runtime_error("the MI355X rasterizer needs device tensors (no CPU path)");
    const int P = (int)scaling.size(0);
    if (scaling.dim() != 2 || scaling.size(1) != 3) throw std::runtime_error("scaling must have dimensions (num_points, 3)");
    if (rotation.dim() != 2 || rotation.size(0) != P || rotation.size(1) != 4)
        throw std::runtime_error("rotation must have dimensions (num_points, 4)");
    const float* sp = param_ptr(scaling, dev, "scaling");
    const float* rp = param_ptr(rotation, dev, "rotation");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    Tensor s = at::empty_like(scaling), q = at::empty_like(rotation);
    if (P && api.r3dgs_activate_params(P, sp, rp, s.data_ptr<float>(), q.data_ptr<float>(), cur_stream(dev)) < 0)
        fail("activate_params");
    return {s, q};
}

// dL_dcodebooks [20,256] from the gradients of the decoded tensors (empty tensor = zeros); the refusals of
// diff_gaussian_rasterization/_C.py _check_quantised_grads
Tensor quantised_codebook_grad(const Tensor& geom_ids, const Tensor& sh_ids, const Tensor& perBandPrimitiveCount,
                               const Tensor& cumSumPrimitiveCount, const Tensor& coeffsNum, const Tensor& dL_dfeatures_dc,
                               const Tensor& dL_dfeatures_rest, const Tensor& dL_dopacity, const Tensor& dL_dscaling,
                               const Tensor& dL_drotation)
{
    need(api.r3dgs_quantised_codebook_grad_workspace_bytes, "r3dgs_quantised_codebook_grad");
    const c10::Device dev = geom_ids.device();
    if (!dev.is_cuda()) throw std::runtime_error("the MI355X rasterizer needs device tensors (no CPU path)");
    if (geom_ids.scalar_type() != at::kByte || geom_ids.dim() != 2 || geom_ids.size(1) != 8)
        throw std::runtime_error("geom_ids must be uint8 with dimensions (num_points, 8)");
    const int64_t P = geom_ids.size(0);
    if (sh_ids.scalar_type() != at::kByte || sh_ids.dim() != 1) throw std::runtime_error("sh_ids must be a flat uint8 tensor");
    auto plain = [&](const Tensor& t, const char* name) {
        if (t.device() != dev) throw std::runtime_error(std::string(name) + ": expected a tensor on " + dev.str() + ", got " + t.device().str());
        if (!t.is_contiguous()) throw std::runtime_error(std::string(name) + ": quantised_codebook_grad needs a contiguous tensor");
    };
    plain(geom_ids, "geom_ids");
    plain(sh_ids, "sh_ids");
    const Tensor* tables[3] = {&perBandPrimitiveCount, &cumSumPrimitiveCount, &coeffsNum};
    const char* table_names[3] = {"perBandPrimitiveCount", "cumSumPrimitiveCount", "coeffsNum"};
    for (int k = 0; k < 3; k++) {
        if (tables[k]->scalar_type() != at::kInt || tables[k]->numel() != 4)
            throw std::runtime_error(std::string(table_names[k]) + " must be int32 with 4 entries (degrees 0..3)");
        plain(*tables[k], table_names[k]);
    }
    const Tensor* grads[5] = {&dL_dfeatures_dc, &dL_dfeatures_rest, &dL_dopacity, &dL_dscaling, &dL_drotation};
    const char* grad_names[5] = {"dL_dfeatures_dc", "dL_dfeatures_rest", "dL_dopacity", "dL_dscaling", "dL_drotation"};
    const std::vector<int64_t> shapes[5] = {{P, 1, 3}, {P, 15, 3}, {P, 1}, {P, 3}, {P, 4}};
    const float* gp[5];
    for (int k = 0; k < 5; k++) {
        const Tensor& t = *grads[k];
        gp[k] = nullptr;
        if (!t.defined() || (t.numel() == 0 && t.dim() == 1)) continue;   // absent: zeros
        if (t.scalar_type() != at::kFloat || t.sizes().vec() != shapes[k])
            throw std::runtime_error(std::string(grad_names[k]) + " must be float32 with the decoder's dimensions (or None)");
        plain(t, grad_names[k]);
        gp[k] = t.numel() ? t.data_ptr<float>() : nullptr;
    }
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    Tensor out = at::empty({20, 256}, geom_ids.options().dtype(at::kFloat));
    Tensor work = at::empty({(int64_t)api.r3dgs_quantised_codebook_grad_workspace_bytes((int)P)}, geom_ids.options());
    if (api.r3dgs_quantised_codebook_grad((int)P, coeffsNum.data_ptr<int>(), perBandPrimitiveCount.data_ptr<int>(),
                                          cumSumPrimitiveCount.data_ptr<int>(), P ? geom_ids.data_ptr<uint8_t>() : nullptr,
                                          sh_ids.numel() ? sh_ids.data_ptr<uint8_t>() : nullptr, gp[0], gp[1], gp[2], gp[3], gp[4],
                                          out.data_ptr<float>(), work.numel() ? work.data_ptr() : nullptr, cur_stream(dev)) < 0)
        fail("quantised_codebook_grad");
    return out;
}

// markVisible (rasterize_points.cu:307-326)
Tensor mark_visible(const Tensor& means3D, const Tensor& viewmatrix, const Tensor& projmatrix)
{
    need_bound();
    const c10::Device dev = means3D.device();
    const int P = (int)means3D.size(0);
    Tensor present = at::zeros({P}, at::TensorOptions().dtype(at::kBool).device(dev));
    if (P) {
        const Tensor m3 = dev_f32(means3D, dev), vm = dev_f32(viewmatrix, dev), pm = dev_f32(projmatrix, dev);
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
        if (api.r3dgs_mark_visible(P, opt_ptr<float>(m3), opt_ptr<float>(vm), opt_ptr<float>(pm),
                               reinterpret_cast<unsigned char*>(present.data_ptr()),
                               cur_stream(dev)) < 0)
            fail("mark_visible");
    }
    return present;
}

// ---- fused L1 + D-SSIM loss (r3dgs_loss.h): the same calls as diff_gaussian_rasterization/_C.py's l1_ssim_* / l1_*;
// r3dgs_loss.py has checked the inputs (device fp32, contiguous, same shape).  Absent optional tensors are empty.

void need_loss() { need(api.r3dgs_l1_ssim_workspace_bytes, "fused loss"); }

// the scratch tensor of a loss call whose size query said ws_bytes; 0 refuses `what`, "<call>: invalid <size>"
Tensor loss_workspace(const char* what, size_t ws_bytes, const c10::Device& dev)
{
    if (ws_bytes == 0) throw std::runtime_error(what);
    return at::empty({(int64_t)ws_bytes}, at::TensorOptions().dtype(at::kByte).device(dev));
}

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> l1_ssim_forward(
    const Tensor& img1, const Tensor& img2, int64_t B, int64_t C, int64_t H, int64_t W, double lambda_dssim, bool want_partials,
    bool want_map)
{
    need_loss();
    const c10::Device dev = img1.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
    Tensor l1 = at::empty({}, f32), ssim = at::empty({}, f32), loss = at::empty({}, f32), dssim = at::empty({}, f32);
    Tensor per_image = at::empty({B}, f32);
    Tensor ssim_map = want_map ? at::empty({B, C, H, W}, f32) : at::empty({0}, f32);
    Tensor partials = want_partials ? at::empty({3, B, C, H, W}, f32) : at::empty({0}, f32);
    Tensor ws = loss_workspace("l1_ssim_forward: invalid shape", api.r3dgs_l1_ssim_workspace_bytes((int)B, (int)C, (int)H, (int)W), dev);
    if (api.r3dgs_l1_ssim_forward((int)B, (int)C, (int)H, (int)W, img1.data_ptr<float>(), img2.data_ptr<float>(),
                                  (float)lambda_dssim, l1.data_ptr<float>(), ssim.data_ptr<float>(), per_image.data_ptr<float>(),
                                  loss.data_ptr<float>(), dssim.data_ptr<float>(), want_map ? ssim_map.data_ptr<float>() : nullptr,
                                  want_partials ? partials.data_ptr<float>() : nullptr, reinterpret_cast<char*>(ws.data_ptr()), cur_stream(dev)) < 0)
        fail("l1_ssim_forward");
    return {l1, ssim, loss, dssim, per_image, ssim_map, partials};
}

Tensor l1_ssim_backward(const Tensor& img1, const Tensor& img2, const Tensor& partials, const Tensor& grad_l1, double coef_l1,
                        const Tensor& grad_ssim, int64_t ssim_grad_mode, double coef_ssim, int64_t B, int64_t C, int64_t H,
                        int64_t W)
{
    need_loss();
    const c10::Device dev = img1.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    Tensor dx = at::empty({B, C, H, W}, at::TensorOptions().dtype(at::kFloat).device(dev));
    if (api.r3dgs_l1_ssim_backward((int)B, (int)C, (int)H, (int)W, img1.data_ptr<float>(), img2.data_ptr<float>(),
                                   opt_ptr<float>(partials), opt_ptr<float>(grad_l1), (float)coef_l1, opt_ptr<float>(grad_ssim),
                                   (int)ssim_grad_mode, (float)coef_ssim, dx.data_ptr<float>(), cur_stream(dev)) < 0)
        fail("l1_ssim_backward");
    return dx;
}

Tensor l1_forward(const Tensor& x, const Tensor& y)
{
    need_loss();
    const c10::Device dev = x.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
    Tensor out = at::empty({}, f32);
    Tensor ws = loss_workspace("l1_forward: invalid element count", api.r3dgs_l1_workspace_bytes(x.numel()), dev);
    if (api.r3dgs_l1_forward(x.numel(), x.data_ptr<float>(), y.data_ptr<float>(), out.data_ptr<float>(),
                             reinterpret_cast<char*>(ws.data_ptr()), cur_stream(dev)) < 0)
        fail("l1_forward");
    return out;
}

Tensor l1_backward(const Tensor& x, const Tensor& y, const Tensor& grad)
{
    need_loss();
    const c10::Device dev = x.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    Tensor dx = at::empty_like(x);
    if (api.r3dgs_l1_backward(x.numel(), x.data_ptr<float>(), y.data_ptr<float>(), grad.data_ptr<float>(), dx.data_ptr<float>(),
                              cur_stream(dev)) < 0)
        fail("l1_backward");
    return dx;
}

// ---- the loss behind an exposure and a mask (r3dgs_loss.h r3dgs_exposure_*): the same calls as _C.py's exposure_*;
// r3dgs_exposure.py has checked the inputs.  An absent exposure or mask is an empty tensor.

void need_exposure() { need(api.r3dgs_exposure_loss_forward, "exposure loss entry points (r3dgs_exposure_loss_forward)"); }

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> exposure_loss_forward(
    const Tensor& img1, const Tensor& img2, const Tensor& exposure, bool exposure_per_image, const Tensor& mask,
    bool mask_per_image, bool mask_target, int64_t B, int64_t C, int64_t H, int64_t W, double lambda_dssim, bool want_partials)
{
    need_exposure();
    const c10::Device dev = img1.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
    Tensor l1 = at::empty({}, f32), ssim = at::empty({}, f32), loss = at::empty({}, f32), dssim = at::empty({}, f32);
    Tensor per_image = at::empty({B}, f32);
    Tensor partials = want_partials ? at::empty({3, B, C, H, W}, f32) : at::empty({0}, f32);
    Tensor ws = loss_workspace("exposure_loss_forward: invalid shape",
                               api.r3dgs_exposure_loss_workspace_bytes((int)B, (int)C, (int)H, (int)W), dev);
    if (api.r3dgs_exposure_loss_forward((int)B, (int)C, (int)H, (int)W, img1.data_ptr<float>(), img2.data_ptr<float>(),
                                        opt_ptr<float>(exposure), (int)exposure_per_image, opt_ptr<float>(mask), (int)mask_per_image,
                                        (int)mask_target, (float)lambda_dssim, l1.data_ptr<float>(), ssim.data_ptr<float>(),
                                        per_image.data_ptr<float>(), loss.data_ptr<float>(), dssim.data_ptr<float>(),
                                        want_partials ? partials.data_ptr<float>() : nullptr, blob_ptr(ws), (size_t)ws.numel(),
                                        cur_stream(dev)) < 0)
        fail("exposure_loss_forward");
    return {l1, ssim, loss, dssim, per_image, partials};
}

std::tuple<Tensor, Tensor> exposure_loss_backward(const Tensor& img1, const Tensor& img2, const Tensor& exposure,
                                                  bool exposure_per_image, const Tensor& mask, bool mask_per_image, bool mask_target,
                                                  const Tensor& partials, const Tensor& grad_loss, double coef_l1, double coef_ssim,
                                                  bool want_exposure_grad, int64_t B, int64_t C, int64_t H, int64_t W)
{
    need_exposure();
    const c10::Device dev = img1.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
    Tensor dx = at::empty({B, C, H, W}, f32);
    Tensor dE = !want_exposure_grad ? at::empty({0}, f32) : (exposure_per_image ? at::empty({B, 3, 4}, f32) : at::empty({3, 4}, f32));
    Tensor ws = loss_workspace("exposure_loss_backward: invalid shape",
                               api.r3dgs_exposure_loss_workspace_bytes((int)B, (int)C, (int)H, (int)W), dev);
    if (api.r3dgs_exposure_loss_backward((int)B, (int)C, (int)H, (int)W, img1.data_ptr<float>(), img2.data_ptr<float>(),
                                         opt_ptr<float>(exposure), (int)exposure_per_image, opt_ptr<float>(mask), (int)mask_per_image,
                                         (int)mask_target, opt_ptr<float>(partials), opt_ptr<float>(grad_loss), (float)coef_l1,
                                         (float)coef_ssim, dx.data_ptr<float>(), want_exposure_grad ? dE.data_ptr<float>() : nullptr,
                                         blob_ptr(ws), (size_t)ws.numel(), cur_stream(dev)) < 0)
        fail("exposure_loss_backward");
    return {dx, dE};
}

Tensor exposure_apply(const Tensor& img, const Tensor& exposure, bool exposure_per_image, bool clamp01, int64_t B, int64_t H, int64_t W)
{
    need(api.r3dgs_exposure_apply, "exposure loss entry points (r3dgs_exposure_loss_forward)");
    const c10::Device dev = img.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    Tensor out = at::empty({B, 3, H, W}, at::TensorOptions().dtype(at::kFloat).device(dev));
    if (api.r3dgs_exposure_apply((int)B, (int)H, (int)W, img.data_ptr<float>(), exposure.data_ptr<float>(), (int)exposure_per_image,
                                 (int)clamp01, out.data_ptr<float>(), cur_stream(dev)) < 0)
        fail("exposure_apply");
    return out;
}

// ---- fused Adam step (r3dgs_optim.h): the same calls as diff_gaussian_rasterization/_C.py's adam_step*; r3dgs_optim.py has
// checked the tensors (one device, fp32, contiguous, matching sizes).  Scalars arrive as doubles and are rounded to fp32 once.

template <class Seg>
constexpr bool is_capturable = std::is_same<Seg, r3dgs_adam_capturable_segment>::value;

// the segments of a step from its tensor lists: six scalars per tensor (r3dgs_adam_segment) or, with steps and lrs, four
// (r3dgs_adam_capturable_segment: lr_value, beta1, beta2, eps; lrs[i] an empty tensor or a 0-d device float32 lr)
template <class Seg>
std::vector<Seg> pack(const char* what, const std::vector<Tensor>& params, const std::vector<Tensor>& grads,
                      const std::vector<Tensor>& exp_avgs, const std::vector<Tensor>& exp_avg_sqs, const std::vector<double>& scalars,
                      const std::vector<Tensor>* steps = nullptr, const std::vector<Tensor>* lrs = nullptr)
{
    constexpr size_t per = is_capturable<Seg> ? 4 : 6;
    const size_t n = params.size();
    if (grads.size() != n || exp_avgs.size() != n || exp_avg_sqs.size() != n || scalars.size() != per * n)
        throw std::runtime_error("adam_step: list lengths differ");
    if (is_capturable<Seg> && (steps->size() != n || lrs->size() != n)) throw std::runtime_error(std::string(what) + ": list lengths differ");
    std::vector<Seg> segs(n);
    for (size_t i = 0; i < n; i++) {
        const double* s = &scalars[per * i];
        float *p = params[i].data_ptr<float>(), *g = grads[i].data_ptr<float>(), *m = exp_avgs[i].data_ptr<float>(),
              *v = exp_avg_sqs[i].data_ptr<float>();
        const long long count = params[i].numel();
        if constexpr (is_capturable<Seg>)
            segs[i] = {p, g, m, v, (*steps)[i].data_ptr<float>(), opt_ptr<float>((*lrs)[i]), count, s[0], s[1], s[2], s[3]};
        else
            segs[i] = {p, g, m, v, count, (float)s[0], (float)s[1], (float)s[2], (float)s[3], (float)s[4], (float)s[5]};
    }
    return segs;
}

// floats per Gaussian of each tensor (the C ABI checks n == P * row_len again)
std::vector<int> row_lens(const std::vector<Tensor>& params, long long P, const char* what)
{
    std::vector<int> out;
    for (const Tensor& t : params) {
        if (t.dim() < 1 || t.size(0) != P)
            throw std::runtime_error(std::string(what) + ": a tensor is not [P, ...] with P = " + std::to_string(P));
        out.push_back(P ? (int)(t.numel() / P) : 1);
    }
    return out;
}

// the dense step of the segments, or -- radii given: the rasterizer's device int32 [P], every tensor [P, ...] -- the
// visibility-gated one
template <class Seg>
void adam_run(const char* what, const std::vector<Tensor>& params, const std::vector<Seg>& segs, const Tensor* radii = nullptr)
{
    const int n = (int)segs.size();
    if (n == 0) return;
    const c10::Device dev = params[0].device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    int st;
    if (radii) {
        const long long P = radii->numel();
        const std::vector<int> lens = row_lens(params, P, what);
        if constexpr (is_capturable<Seg>)
            st = api.r3dgs_adam_step_capturable_visible(n, segs.data(), lens.data(), opt_ptr<int>(*radii), P, cur_stream(dev));
        else
            st = api.r3dgs_adam_step_visible(n, segs.data(), lens.data(), opt_ptr<int>(*radii), P, cur_stream(dev));
    } else if constexpr (is_capturable<Seg>) {
        st = api.r3dgs_adam_step_capturable(n, segs.data(), cur_stream(dev));
    } else {
        st = api.r3dgs_adam_step(n, segs.data(), cur_stream(dev));
    }
    if (st < 0) fail(what);
}

void adam_step(const std::vector<Tensor>& params, const std::vector<Tensor>& grads, const std::vector<Tensor>& exp_avgs,
               const std::vector<Tensor>& exp_avg_sqs, const std::vector<double>& scalars)
{
    need(api.r3dgs_adam_step, "fused Adam");
    adam_run("adam_step", params, pack<r3dgs_adam_segment>("adam_step", params, grads, exp_avgs, exp_avg_sqs, scalars));
}

void adam_step_capturable(const std::vector<Tensor>& params, const std::vector<Tensor>& grads, const std::vector<Tensor>& exp_avgs,
                          const std::vector<Tensor>& exp_avg_sqs, const std::vector<Tensor>& steps, const std::vector<Tensor>& lrs,
                          const std::vector<double>& scalars)
{
    need(api.r3dgs_adam_step_capturable, "fused Adam");
    adam_run("adam_step_capturable", params,
             pack<r3dgs_adam_capturable_segment>("adam_step_capturable", params, grads, exp_avgs, exp_avg_sqs, scalars, &steps, &lrs));
}

void adam_step_visible(const std::vector<Tensor>& params, const std::vector<Tensor>& grads, const std::vector<Tensor>& exp_avgs,
                       const std::vector<Tensor>& exp_avg_sqs, const std::vector<double>& scalars, const Tensor& radii)
{
    need(api.r3dgs_adam_step_visible, "visibility-gated Adam");
    adam_run("adam_step_visible", params, pack<r3dgs_adam_segment>("adam_step_visible", params, grads, exp_avgs, exp_avg_sqs, scalars),
             &radii);
}

void adam_step_capturable_visible(const std::vector<Tensor>& params, const std::vector<Tensor>& grads,
                                  const std::vector<Tensor>& exp_avgs, const std::vector<Tensor>& exp_avg_sqs,
                                  const std::vector<Tensor>& steps, const std::vector<Tensor>& lrs,
                                  const std::vector<double>& scalars, const Tensor& radii)
{
    need(api.r3dgs_adam_step_capturable_visible, "visibility-gated Adam");
    adam_run("adam_step_capturable_visible", params,
             pack<r3dgs_adam_capturable_segment>("adam_step_capturable_visible", params, grads, exp_avgs, exp_avg_sqs, scalars, &steps,
                                                 &lrs),
             &radii);
}

// ---- per-iteration training statistics (r3dgs_trainstats.h): the same calls as diff_gaussian_rasterization/_C.py's
// visible_means / alpha_regul_backward / densification_stats; r3dgs_train_stats.py has checked the tensors (one device, dtypes,
// shapes, contiguity).  Absent optional tensors are empty.

void need_stats() { need(api.r3dgs_train_stats_workspace_bytes, "training statistics"); }

// -> (visibility bool[P], n_visible int32 0-d, alpha_mean fp32 0-d, sh_abs_mean fp32 0-d); a mean that was not asked for (want_alpha /
// want_sh false) comes back as an empty tensor.  features_rest may be empty with want_sh set: M == 1, the mean of nothing.
std::tuple<Tensor, Tensor, Tensor, Tensor> visible_means(const Tensor& radii, const Tensor& opacity, const Tensor& features_rest,
                                                         bool want_alpha, bool want_sh, int64_t M)
{
    need_stats();
    const c10::Device dev = radii.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
    const int64_t P = radii.numel();
    Tensor vis = at::empty({P}, f32.dtype(at::kBool));
    if (P == 0) {
        const float nan = std::numeric_limits<float>::quiet_NaN();
        return {vis, at::zeros({}, f32.dtype(at::kInt)), want_alpha ? at::full({}, nan, f32) : at::empty({0}, f32),
                want_sh ? at::full({}, nan, f32) : at::empty({0}, f32)};
    }
    Tensor n = at::empty({}, f32.dtype(at::kInt));
    Tensor alpha = want_alpha ? at::empty({}, f32) : at::empty({0}, f32);
    Tensor sh = want_sh ? at::empty({}, f32) : at::empty({0}, f32);
    Tensor ws = at::empty({(int64_t)api.r3dgs_train_stats_workspace_bytes((int)P)}, f32.dtype(at::kByte));
    if (api.r3dgs_visible_means((int)P, (int)M, radii.data_ptr<int>(), opt_ptr<float>(opacity), opt_ptr<float>(features_rest),
                                reinterpret_cast<uint8_t*>(vis.data_ptr()), n.data_ptr<int>(), want_alpha ? alpha.data_ptr<float>() : nullptr,
                                want_sh ? sh.data_ptr<float>() : nullptr, reinterpret_cast<char*>(ws.data_ptr()), cur_stream(dev)) < 0)
        fail("visible_means");
    return {vis, n, alpha, sh};
}

void alpha_regul_backward(const Tensor& radii, const Tensor& opacity, const Tensor& upstream, const Tensor& n_visible, Tensor& grad)
{
    need_stats();
    if (radii.numel() == 0) return;
    const c10::Device dev = radii.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    if (api.r3dgs_alpha_regul_backward((int)radii.numel(), radii.data_ptr<int>(), opacity.data_ptr<float>(), upstream.data_ptr<float>(),
                                       n_visible.data_ptr<int>(), grad.data_ptr<float>(), cur_stream(dev)) < 0)
        fail("alpha_regul_backward");
}

void densification_stats(const Tensor& viewspace_grad, const Tensor& radii, Tensor& xyz_gradient_accum, Tensor& denom,
                         Tensor& max_radii2D)
{
    need_stats();
    if (radii.numel() == 0) return;
    const c10::Device dev = radii.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    if (api.r3dgs_densification_stats((int)radii.numel(), viewspace_grad.data_ptr<float>(), radii.data_ptr<int>(),
                                      xyz_gradient_accum.data_ptr<float>(), denom.data_ptr<float>(), max_radii2D.data_ptr<float>(),
                                      cur_stream(dev)) < 0)
        fail("densification_stats");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "compiled torch binding of libr3dgs_hip.so's hot calls (see diff_gaussian_rasterization/_C.py)";
    m.def("bind", &bind);
    m.def("entry_points", &entry_points);
    m.def("forward_reserved", &forward_reserved);
    m.def("backward", &backward);
    m.def("backward_absgrad", &backward_absgrad);
    m.def("mark_visible", &mark_visible);
    m.def("aux_maps", &aux_maps);
    m.def("contribution_scores", &contribution_scores);
    m.def("forward_params", &forward_params);
    m.def("forward_params_reserved", &forward_params_reserved);
    m.def("backward_params", &backward_params);
    m.def("backward_params_absgrad", &backward_params_absgrad);
    m.def("activate_params", &activate_params);
    m.def("quantised_codebook_grad", &quantised_codebook_grad);
    m.def("l1_ssim_forward", &l1_ssim_forward);
    m.def("l1_ssim_backward", &l1_ssim_backward);
    m.def("l1_forward", &l1_forward);
    m.def("l1_backward", &l1_backward);
    m.def("exposure_loss_forward", &exposure_loss_forward);
    m.def("exposure_loss_backward", &exposure_loss_backward);
    m.def("exposure_apply", &exposure_apply);
    m.def("adam_step", &adam_step);
    m.def("adam_step_capturable", &adam_step_capturable);
    m.def("adam_step_visible", &adam_step_visible);
    m.def("adam_step_capturable_visible", &adam_step_capturable_visible);
    m.def("visible_means", &visible_means);
    m.def("alpha_regul_backward", &alpha_regul_backward);
    m.def("densification_stats", &densification_stats);
    m.def("library_version", []() {
        need_bound();
        return std::string(api.r3dgs_version());
    });
}
