// PyTorch-ROCm custom-op registration of the hot-path kernels: TORCH_LIBRARY(sfm_hip, ...).
//
// This is the thin torch-facing layer ABOVE the C ABI of include/sfm_hip.h (which stays free of torch types):
// every op checks its tensors, takes the current HIP stream from torch and calls the matching sfm_* entry point
// of libsfm_hip.so.  The TORCH_LIBRARY(sfm_hip, m) block below is the list of ops.  An op is an in-place form `x_out`
// over the caller's buffers (`x_` in the schema; what the pre-allocating engine calls), a functional form
// `x_new(bool meta, ...)` that allocates the outputs and, unless `meta`, fills them, or both; the device and the Meta
// registration of each come from that one function (Forms, Noop).
//
// Built by structure_from_motion_amd/build.py into csrc/libsfm_torch_ops.so (host code only: no kernels here).
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <cmath>
#include <tuple>
#include <vector>

#include "../../include/sfm_hip.h"
#include "sfm_loss.h"   // sfmloss::scale_ok alone: the rest of it is for the HIP compiler

namespace {

using at::Tensor;

// Every op runs on the device of its first tensor argument (sample_philox: of its `device` argument), not on whatever
// device happens to be current: OpDevice makes that device current for the op's duration (the C ABI launches on the
// current device), current_stream() is that device's current torch stream, and need() refuses a tensor that lives
// elsewhere — a kernel handed pointers of two GPUs would fault or race.  A Meta form (`meta`) runs nothing and has no device.
thread_local const c10::Device* g_op_device = nullptr;

struct OpDevice {
    c10::Device device;
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard;
    const c10::Device* outer;
    explicit OpDevice(const c10::Device& d, bool meta = false) : device(d), outer(g_op_device) {
        if (meta) return;
        TORCH_CHECK(d.is_cuda(), "sfm_hip: expected a ROCm device, got ", d);
        guard.set_device(d);
        g_op_device = &device;
    }
    explicit OpDevice(const Tensor& first, bool meta = false) : OpDevice(first.device(), meta) {}
    ~OpDevice() { g_op_device = outer; }
    OpDevice(const OpDevice&) = delete;
    OpDevice& operator=(const OpDevice&) = delete;
};

void* current_stream() {
    return (void*)c10::hip::getCurrentHIPStream(g_op_device ? g_op_device->index() : (c10::DeviceIndex)-1).stream();
}

void ok(int status, const char* what) {
    TORCH_CHECK(status == SFM_OK, what, " failed (", status, "): ", sfm_last_error());
}

void need(const Tensor& t, const char* name, at::ScalarType dtype) {
    TORCH_CHECK(t.is_cuda(), "sfm_hip: ", name, " must be a ROCm device tensor");
    TORCH_CHECK(g_op_device == nullptr || t.device() == *g_op_device, "sfm_hip: ", name, " is on ", t.device(),
                " but the op runs on ", *g_op_device, ": all tensor arguments must live on one device");
    TORCH_CHECK(t.scalar_type() == dtype, "sfm_hip: ", name, " must have dtype ", dtype, ", got ", t.scalar_type());
    TORCH_CHECK(t.is_contiguous(), "sfm_hip: ", name, " must be contiguous");
}

template <typename T>
T* ptr(const Tensor& t) {
    return t.numel() ? static_cast<T*>(t.data_ptr()) : nullptr;
}

template <typename T>
T* ptr(const std::optional<Tensor>& t) {
    return t.has_value() && t->defined() ? ptr<T>(*t) : nullptr;
}

at::TensorOptions like(const Tensor& t, at::ScalarType dtype) { return t.options().dtype(dtype); }

// A new tensor beside `t`.  Its sizes are SymInt, taken with sym_size(): a functional form states each output's shape once,
// for real tensors and for fake ones (under dynamic-shape tracing sizes are symbolic, and size() / sizes() / numel() are
// not available: value checks stay with the in-place forms).
using c10::SymInt;

Tensor alloc(const Tensor& t, at::ScalarType dtype, std::initializer_list<SymInt> shape) {
    return at::empty_symint(c10::SymIntArrayRef(shape.begin(), shape.size()), like(t, dtype));
}

// The two registrations of a functional form x_new(bool meta, ...): Forms<&x_new>::call<false> under the device key,
// call<true> under Meta
template <auto Fn>
struct Forms;
template <typename R, typename... A, R (*Fn)(bool, A...)>
struct Forms<Fn> {
    template <bool META>
    static R call(A... a) {
        return Fn(META, std::forward<A>(a)...);
    }
};

// The Meta registration of an in-place form x_out: its parameter list and nothing to do, the caller's buffers fix every shape
template <auto Fn>
struct Noop;
template <typename... A, void (*Fn)(A...)>
struct Noop<Fn> {
    static void call(A...) {}
};

constexpr int64_t kRecordWords = sizeof(sfm_select_result) / 8;

// ---- shape helpers --------------------------------------------------------------------------------------------
struct Dims {
    int64_t batch, n, h;
};

Dims corr_dims(const Tensor& corr) {
    TORCH_CHECK(corr.dim() == 3 && corr.size(2) == 4, "sfm_hip: corr must be [batch, n, 4]");
    return {corr.size(0), corr.size(1), 0};
}

Dims hypothesis_dims(const Tensor& corr, const Tensor& S) {
    Dims d = corr_dims(corr);
    TORCH_CHECK(S.dim() == 3 && S.size(0) == d.batch && S.size(2) == 8, "sfm_hip: S must be [batch, h, 8]");
    d.h = S.size(1);
    return d;
}

void check_E(const Tensor& E, const Dims& d) {
    TORCH_CHECK(E.dim() == 3 && E.size(0) == d.batch && E.size(1) == d.h && E.size(2) == 9,
                "sfm_hip: E must be [batch, h, 9]");
}

// ---- normalize_coords ------------------------------------------------------------------------------------------
void normalize_coords_out(const Tensor& pix_a, const Tensor& pix_b, double fx, double fy, double cx, double cy,
                          Tensor& out) {
    const OpDevice scope(pix_a);
    need(pix_a, "pix_a", at::kDouble);
    need(pix_b, "pix_b", at::kDouble);
    need(out, "out", at::kDouble);
    TORCH_CHECK(pix_a.sizes() == pix_b.sizes() && pix_a.dim() >= 1 && pix_a.size(-1) == 2,
                "sfm_hip: pix_a, pix_b must be [..., 2] of equal shape");
    const int64_t count = pix_a.numel() / 2;
    TORCH_CHECK(out.numel() == 4 * count, "sfm_hip: out must hold 4 doubles per correspondence");
    ok(sfm_normalize_correspondences(ptr<double>(pix_a), ptr<double>(pix_b), count, fx, fy, cx, cy, ptr<double>(out),
                                     current_stream()),
       "sfm_normalize_correspondences");
}

Tensor normalize_coords_new(bool meta, const Tensor& pix_a, const Tensor& pix_b, double fx, double fy, double cx, double cy) {
    TORCH_CHECK(pix_a.dim() >= 1 && (meta ? pix_a.dim() == pix_b.dim() : pix_a.size(-1) == 2),
                meta ? "sfm_hip: pix_a, pix_b must be [..., 2] of equal shape" : "sfm_hip: pix_a must be [..., 2]");
    std::vector<SymInt> shape(pix_a.sym_sizes().begin(), pix_a.sym_sizes().end());
    shape.back() = 4;
    Tensor out = at::empty_symint(shape, pix_a.options());
    if (!meta) normalize_coords_out(pix_a, pix_b, fx, fy, cx, cy, out);
    return out;
}

// ---- sample_philox ---------------------------------------------------------------------------------------------
// seeds travel as int64 (torch schemas have no uint64): the bit pattern is the Philox key
Tensor sample_philox(int64_t seed, int64_t seed_stride, int64_t h_begin, int64_t h_count, int64_t n, int64_t batch,
                     at::Device device) {
    TORCH_CHECK(device.is_cuda(), "sfm_hip::sample_philox: device must be a ROCm device");
    const OpDevice scope(device);
    Tensor S = at::empty({batch, h_count, 8}, at::TensorOptions().dtype(at::kInt).device(device));
    ok(sfm_sample_philox((uint64_t)seed, (uint64_t)seed_stride, h_begin, h_count, n, batch, ptr<int32_t>(S),
                         current_stream()),
       "sfm_sample_philox");
    return S;
}

// ---- fit_eight_point and five_point_fit (six-item samples, sfm_five_point.hip): one body, the entry point differs ----
using EssentialFit = int (*)(const double*, int64_t, const int32_t*, int64_t, int64_t, double*, int32_t*, void*);

int fit_eight_point_entry(const double* corr, int64_t n, const int32_t* S, int64_t h, int64_t batch, double* E, int32_t* flags,
                          void* stream) {
    return sfm_fit_eight_point(corr, n, S, h, batch, E, flags, nullptr, stream);
}

void essential_fit(EssentialFit entry, const char* name, const Tensor& corr, const Tensor& S, Tensor& E, Tensor& flags) {
    const OpDevice scope(corr);
    need(corr, "corr", at::kDouble);
    need(S, "S", at::kInt);
    need(E, "E", at::kDouble);
    need(flags, "flags", at::kInt);
    const Dims d = hypothesis_dims(corr, S);
    check_E(E, d);
    TORCH_CHECK(flags.numel() == d.batch * d.h, "sfm_hip: flags must be [batch, h]");
    ok(entry(ptr<double>(corr), d.n, ptr<int32_t>(S), d.h, d.batch, ptr<double>(E), ptr<int32_t>(flags), current_stream()), name);
}

void fit_eight_point_out(const Tensor& corr, const Tensor& S, Tensor& E, Tensor& flags) {
    essential_fit(fit_eight_point_entry, "sfm_fit_eight_point", corr, S, E, flags);
}

void five_point_fit_out(const Tensor& corr, const Tensor& S, Tensor& E, Tensor& flags) {
    essential_fit(sfm_five_point_fit, "sfm_five_point_fit", corr, S, E, flags);
}

// what a functional form over corr and S checks before it allocates: the ranks, and on the device the other sizes
void fit_dims(bool meta, const Tensor& corr, const Tensor& S) {
    TORCH_CHECK(corr.dim() == 3, "sfm_hip: corr must be [batch, n, 4]");
    TORCH_CHECK(S.dim() == 3, "sfm_hip: S must be [batch, h, 8]");
    if (!meta) hypothesis_dims(corr, S);
}

// the allocating form of an in-place fit
template <void (*FitOut)(const Tensor&, const Tensor&, Tensor&, Tensor&)>
std::tuple<Tensor, Tensor> essential_fit_new(bool meta, const Tensor& corr, const Tensor& S) {
    fit_dims(meta, corr, S);
    Tensor E = alloc(corr, at::kDouble, {corr.sym_size(0), S.sym_size(1), 9});
    Tensor flags = alloc(corr, at::kInt, {corr.sym_size(0), S.sym_size(1)});
    if (!meta) FitOut(corr, S, E, flags);
    return {E, flags};
}

// The tensors every whole-pass op takes, checked: `items` ("corr" / "pts") and `model` ("E" / "model") by their names in the
// op; the shape of `model` is left to the caller.
Dims pass_checks(const Tensor& items, const char* items_name, Dims (*dims)(const Tensor&, const Tensor&), const Tensor& S,
                 const Tensor& model, const char* model_name, const Tensor& flags, const Tensor& cnt, const Tensor& s1, const Tensor& s2,
                 const Tensor& result, const std::optional<Tensor>& mask) {
    need(items, items_name, at::kDouble);
    need(S, "S", at::kInt);
    need(model, model_name, at::kDouble);
    need(flags, "flags", at::kInt);
    need(cnt, "cnt", at::kInt);
    need(s1, "s1", at::kDouble);
    need(s2, "s2", at::kDouble);
    need(result, "result", at::kLong);
    if (mask.has_value()) need(*mask, "mask", at::kByte);
    const Dims d = dims(items, S);
    TORCH_CHECK(flags.numel() == d.batch * d.h && cnt.numel() == d.batch * d.h && s1.numel() == d.batch * d.h &&
                    s2.numel() == d.batch * d.h,
                "sfm_hip: flags, cnt, s1, s2 must be [batch, h]");
    TORCH_CHECK(result.numel() == d.batch * kRecordWords, "sfm_hip: result must be int64 [batch, 5]");
    TORCH_CHECK(!mask.has_value() || mask->numel() == d.batch * d.n, "sfm_hip: mask must be uint8 [batch, n]");
    return d;
}

// the whole five-point pass (sfm_five_point_ransac_pass): fit (from S, or Philox-sampled with use_philox), six-item scoring,
// selection and the optional mask
void five_point_ransac_pass_out(const Tensor& corr, int64_t seed, int64_t seed_stride, bool use_philox, int64_t h_begin, double thr,
                                double min_extra, int64_t aggregation, Tensor& S, Tensor& E, Tensor& flags, Tensor& cnt, Tensor& s1,
                                Tensor& s2, Tensor& result, const std::optional<Tensor>& mask) {
    const OpDevice scope(corr);
    const Dims d = pass_checks(corr, "corr", hypothesis_dims, S, E, "E", flags, cnt, s1, s2, result, mask);
    check_E(E, d);
    ok(sfm_five_point_ransac_pass((uint64_t)seed, (uint64_t)seed_stride, use_philox ? 1 : 0, h_begin, ptr<double>(corr), d.n, d.h,
                                  d.batch, thr, min_extra, (int)aggregation, ptr<int32_t>(S), ptr<double>(E), ptr<int32_t>(flags),
                                  ptr<int32_t>(cnt), ptr<double>(s1), ptr<double>(s2),
                                  reinterpret_cast<sfm_select_result*>(ptr<int64_t>(result)), ptr<uint8_t>(mask), current_stream()),
       "sfm_five_point_ransac_pass");
}

// Philox sampling fused into the fit launch; `seed_dev` (int64 [1] on the device) is read at kernel run time when given
void sample_fit_philox_out(const Tensor& corr, int64_t seed, const std::optional<Tensor>& seed_dev, int64_t seed_stride,
                           int64_t h_begin, Tensor& S, Tensor& E, Tensor& flags) {
    const OpDevice scope(corr);
    need(corr, "corr", at::kDouble);
    need(S, "S", at::kInt);
    need(E, "E", at::kDouble);
    need(flags, "flags", at::kInt);
    if (seed_dev.has_value()) need(*seed_dev, "seed_dev", at::kLong);
    const Dims d = hypothesis_dims(corr, S);
    check_E(E, d);
    ok(sfm_sample_fit_philox((uint64_t)seed, reinterpret_cast<const uint64_t*>(ptr<int64_t>(seed_dev)),
                             (uint64_t)seed_stride, h_begin, ptr<double>(corr), d.n, d.h, d.batch, ptr<int32_t>(S),
                             ptr<double>(E), ptr<int32_t>(flags), current_stream()),
       "sfm_sample_fit_philox");
}

// ---- score_sed -------------------------------------------------------------------------------------------------
void score_sed_out(const Tensor& corr, const Tensor& E, const Tensor& S, double thr, Tensor& cnt, Tensor& s1, Tensor& s2,
                   const std::optional<Tensor>& workspace) {
    const OpDevice scope(corr);
    need(corr, "corr", at::kDouble);
    need(E, "E", at::kDouble);
    need(S, "S", at::kInt);
    need(cnt, "cnt", at::kInt);
    need(s1, "s1", at::kDouble);
    need(s2, "s2", at::kDouble);
    const Dims d = hypothesis_dims(corr, S);
    check_E(E, d);
    TORCH_CHECK(cnt.numel() == d.batch * d.h && s1.numel() == cnt.numel() && s2.numel() == cnt.numel(),
                "sfm_hip: cnt, s1, s2 must be [batch, h]");
    int64_t ws_bytes = 0;
    if (workspace.has_value() && workspace->defined()) {
        need(*workspace, "workspace", at::kByte);
        ws_bytes = workspace->numel();
    }
    ok(sfm_score_sed(ptr<double>(corr), d.n, ptr<double>(E), ptr<int32_t>(S), d.h, d.batch, thr, ptr<int32_t>(cnt),
                     ptr<double>(s1), ptr<double>(s2), ptr<unsigned char>(workspace), ws_bytes, current_stream()),
       "sfm_score_sed");
}

// exact = the all-fp64 kernel; otherwise the two-tier kernel (needs a scratch buffer, allocated here)
std::tuple<Tensor, Tensor, Tensor> score_sed_new(bool meta, const Tensor& corr, const Tensor& E, const Tensor& S, double thr,
                                                 bool exact) {
    fit_dims(meta, corr, S);
    TORCH_CHECK(E.dim() == 3, "sfm_hip: E must be [batch, h, 9]");
    const SymInt b = corr.sym_size(0), h = S.sym_size(1);
    Tensor cnt = alloc(corr, at::kInt, {b, h}), s1 = alloc(corr, at::kDouble, {b, h}), s2 = alloc(corr, at::kDouble, {b, h});
    if (meta) return {cnt, s1, s2};
    std::optional<Tensor> workspace;
    if (!exact) workspace = at::empty({sfm_score_workspace_bytes(corr.size(1), S.size(1), corr.size(0))}, like(corr, at::kByte));
    score_sed_out(corr, E, S, thr, cnt, s1, s2, workspace);
    return {cnt, s1, s2};
}

// ---- fused small pass (two launches: fit + workspace preparation, scoring + selection + mask) -------------------
using PassEntry = int (*)(uint64_t, const uint64_t*, int, int64_t, const double*, int64_t, int64_t, double, double, int, int64_t,
                          int32_t*, double*, int32_t*, int32_t*, double*, double*, sfm_select_result*, uint8_t*, void*, int64_t,
                          void*, const sfm_score_options*);
template <PassEntry ENTRY>
void ransac_pass_out(const char* name, const Tensor& corr, int64_t seed, const std::optional<Tensor>& seed_dev, bool use_philox,
                     int64_t h_begin, double thr, double min_extra, int64_t aggregation, int64_t h_offset,
                     Tensor& S, Tensor& E, Tensor& flags, Tensor& cnt, Tensor& s1, Tensor& s2, Tensor& result,
                     const std::optional<Tensor>& mask, Tensor& workspace) {
    const OpDevice scope(corr);
    need(corr, "corr", at::kDouble);
    need(S, "S", at::kInt);
    need(E, "E", at::kDouble);
    need(flags, "flags", at::kInt);
    need(cnt, "cnt", at::kInt);
    need(s1, "s1", at::kDouble);
    need(s2, "s2", at::kDouble);
    need(result, "result", at::kLong);
    need(workspace, "workspace", at::kByte);
    if (seed_dev.has_value()) need(*seed_dev, "seed_dev", at::kLong);
    if (mask.has_value()) need(*mask, "mask", at::kByte);
    const Dims d = hypothesis_dims(corr, S);
    TORCH_CHECK(d.batch == 1, "sfm_hip::", name, "_: one image pair per call");
    check_E(E, d);
    TORCH_CHECK(flags.numel() == d.h && cnt.numel() == d.h && s1.numel() == d.h && s2.numel() == d.h,
                "sfm_hip: flags, cnt, s1, s2 must be [1, h]");
    TORCH_CHECK(result.numel() == kRecordWords, "sfm_hip: result must be int64 [1, 5]");
    TORCH_CHECK(!mask.has_value() || mask->numel() == d.n, "sfm_hip: mask must be uint8 [1, n]");
    ok(ENTRY((uint64_t)seed, reinterpret_cast<const uint64_t*>(ptr<int64_t>(seed_dev)), use_philox ? 1 : 0,
             h_begin, ptr<double>(corr), d.n, d.h, thr, min_extra, (int)aggregation, h_offset,
             ptr<int32_t>(S), ptr<double>(E), ptr<int32_t>(flags), ptr<int32_t>(cnt), ptr<double>(s1),
             ptr<double>(s2), reinterpret_cast<sfm_select_result*>(ptr<int64_t>(result)),
             ptr<uint8_t>(mask), ptr<unsigned char>(workspace), workspace.numel(), current_stream(), nullptr),
       name);
}
void ransac_pass_small_out(const Tensor& corr, int64_t seed, const std::optional<Tensor>& seed_dev, bool use_philox,
                           int64_t h_begin, double thr, double min_extra, int64_t aggregation, int64_t h_offset,
                           Tensor& S, Tensor& E, Tensor& flags, Tensor& cnt, Tensor& s1, Tensor& s2, Tensor& result,
                           const std::optional<Tensor>& mask, Tensor& workspace) {
    ransac_pass_out<&sfm_ransac_pass_small>("sfm_ransac_pass_small", corr, seed, seed_dev, use_philox, h_begin, thr, min_extra,
                                            aggregation, h_offset, S, E, flags, cnt, s1, s2, result, mask, workspace);
}
// ---- fused large pass (eight launches: see sfm_hip.h) ------------------------------------------------------------
void ransac_pass_large_out(const Tensor& corr, int64_t seed, const std::optional<Tensor>& seed_dev, bool use_philox,
                           int64_t h_begin, double thr, double min_extra, int64_t aggregation, int64_t h_offset,
                           Tensor& S, Tensor& E, Tensor& flags, Tensor& cnt, Tensor& s1, Tensor& s2, Tensor& result,
                           const std::optional<Tensor>& mask, Tensor& workspace) {
    ransac_pass_out<&sfm_ransac_pass_large>("sfm_ransac_pass_large", corr, seed, seed_dev, use_philox, h_begin, thr, min_extra,
                                            aggregation, h_offset, S, E, flags, cnt, s1, s2, result, mask, workspace);
}

// ---- select_best -----------------------------------------------------------------------------------------------
void select_best_out(const Tensor& cnt, const Tensor& s1, const Tensor& s2, const std::optional<Tensor>& flags,
                     double min_extra, int64_t aggregation, int64_t h_offset, Tensor& result, int64_t sample_size) {
    const OpDevice scope(cnt);
    need(cnt, "cnt", at::kInt);
    need(s1, "s1", at::kDouble);
    need(s2, "s2", at::kDouble);
    need(result, "result", at::kLong);
    if (flags.has_value()) need(*flags, "flags", at::kInt);
    TORCH_CHECK(cnt.dim() == 2 && s1.sizes() == cnt.sizes() && s2.sizes() == cnt.sizes(),
                "sfm_hip: cnt, s1, s2 must be [batch, h]");
    TORCH_CHECK(result.numel() == cnt.size(0) * kRecordWords, "sfm_hip: result must be int64 [batch, 5]");
    ok(sfm_select_best(ptr<int32_t>(cnt), ptr<double>(s1), ptr<double>(s2), ptr<int32_t>(flags), cnt.size(1),
                       cnt.size(0), min_extra, (int)aggregation, h_offset, (int)sample_size,
                       reinterpret_cast<sfm_select_result*>(ptr<int64_t>(result)), current_stream()),
       "sfm_select_best");
}

Tensor select_best_new(bool meta, const Tensor& cnt, const Tensor& s1, const Tensor& s2, const std::optional<Tensor>& flags,
                       double min_extra, int64_t aggregation, int64_t h_offset, int64_t sample_size) {
    TORCH_CHECK(cnt.dim() == 2, "sfm_hip: cnt must be [batch, h]");
    Tensor result = alloc(cnt, at::kLong, {cnt.sym_size(0), kRecordWords});
    if (!meta) select_best_out(cnt, s1, s2, flags, min_extra, aggregation, h_offset, result, sample_size);
    return result;
}

// ---- inlier_mask -----------------------------------------------------------------------------------------------
void inlier_mask_out(const Tensor& corr, const Tensor& E, const Tensor& S, const Tensor& result, double thr,
                     Tensor& mask, int64_t sample_size) {
    const OpDevice scope(corr);
    need(corr, "corr", at::kDouble);
    need(E, "E", at::kDouble);
    need(S, "S", at::kInt);
    need(result, "result", at::kLong);
    need(mask, "mask", at::kByte);
    const Dims d = hypothesis_dims(corr, S);
    check_E(E, d);
    TORCH_CHECK(result.numel() == d.batch * kRecordWords, "sfm_hip: result must be int64 [batch, 5]");
    TORCH_CHECK(mask.numel() == d.batch * d.n, "sfm_hip: mask must be uint8 [batch, n]");
    ok(sfm_inlier_mask(ptr<double>(corr), d.n, ptr<double>(E), ptr<int32_t>(S), d.h, d.batch,
                       reinterpret_cast<const sfm_select_result*>(ptr<int64_t>(result)), thr, (int)sample_size,
                       ptr<uint8_t>(mask), current_stream()),
       "sfm_inlier_mask");
}

Tensor inlier_mask_new(bool meta, const Tensor& corr, const Tensor& E, const Tensor& S, const Tensor& result, double thr,
                       int64_t sample_size) {
    TORCH_CHECK(corr.dim() == 3, "sfm_hip: corr must be [batch, n, 4]");
    if (!meta) corr_dims(corr);
    Tensor mask = alloc(corr, at::kByte, {corr.sym_size(0), corr.sym_size(1)});
    if (!meta) inlier_mask_out(corr, E, S, result, thr, mask, sample_size);
    return mask;
}

// ---- cheirality / triangulate: no in-place form, the device's checks and the launch are in the functional one ---------
Tensor cheirality_new(bool meta, const Tensor& corr, const Tensor& pose_rt, double distance_threshold) {
    const OpDevice scope(corr, meta);
    if (meta) {
        TORCH_CHECK(corr.dim() == 2 && pose_rt.dim() == 2, "sfm_hip: corr [m, 4], pose_rt [poses, 12]");
    } else {
        need(corr, "corr", at::kDouble);
        need(pose_rt, "pose_rt", at::kDouble);
        TORCH_CHECK(corr.dim() == 2 && corr.size(1) == 4, "sfm_hip: corr must be [m, 4]");
        TORCH_CHECK(pose_rt.dim() == 2 && pose_rt.size(1) == 12, "sfm_hip: pose_rt must be [poses, 12]");
    }
    Tensor pass = alloc(corr, at::kByte, {pose_rt.sym_size(0), corr.sym_size(0)});
    if (!meta)
        ok(sfm_cheirality(ptr<double>(corr), corr.size(0), ptr<double>(pose_rt), pose_rt.size(0), distance_threshold,
                          ptr<uint8_t>(pass), current_stream()),
           "sfm_cheirality");
    return pass;
}

Tensor triangulate_new(bool meta, const Tensor& corr, const Tensor& P1, const Tensor& P2) {
    const OpDevice scope(corr, meta);
    if (!meta) {
        need(corr, "corr", at::kDouble);
        need(P1, "P1", at::kDouble);
        need(P2, "P2", at::kDouble);
    }
    TORCH_CHECK(corr.dim() == 2 && (meta || corr.size(1) == 4), "sfm_hip: corr must be [m, 4]");
    if (!meta) TORCH_CHECK(P1.numel() == 12 && P2.numel() == 12, "sfm_hip: P1, P2 must hold 12 doubles (rows 0..2, 4 columns)");
    Tensor X = at::empty_symint({corr.sym_size(0), 3}, corr.options());
    if (!meta)
        ok(sfm_triangulate(ptr<double>(corr), corr.size(0), ptr<double>(P1), ptr<double>(P2), ptr<double>(X),
                           current_stream()),
           "sfm_triangulate");
    return X;
}


// ---- homography (sfm_homography.hip): corr [batch, n, 4], S [batch, h, 8] (first 4 entries used), H [batch, h, 9] ----------
void check_H(const Tensor& H, const Dims& d) {
    TORCH_CHECK(H.dim() == 3 && H.size(0) == d.batch && H.size(1) == d.h && H.size(2) == 9, "sfm_hip: H must be [batch, h, 9]");
}

void homography_fit_out(const Tensor& corr, const Tensor& S, Tensor& H, Tensor& flags) {
    essential_fit(sfm_homography_fit, "sfm_homography_fit", corr, S, H, flags);
}

// no in-place form of these two: the device's checks and the launch are in the functional one
std::tuple<Tensor, Tensor, Tensor> homography_score_new(bool meta, const Tensor& corr, const Tensor& H, const Tensor& S, double thr) {
    const OpDevice scope(corr, meta);
    if (!meta) {
        need(corr, "corr", at::kDouble);
        need(H, "H", at::kDouble);
        need(S, "S", at::kInt);
    }
    fit_dims(meta, corr, S);
    TORCH_CHECK(H.dim() == 3, "sfm_hip: H must be [batch, h, 9]");
    const SymInt b = corr.sym_size(0), h = S.sym_size(1);
    Tensor cnt = alloc(corr, at::kInt, {b, h}), s1 = alloc(corr, at::kDouble, {b, h}), s2 = alloc(corr, at::kDouble, {b, h});
    if (meta) return {cnt, s1, s2};
    const Dims d = hypothesis_dims(corr, S);
    check_H(H, d);
    ok(sfm_homography_score(ptr<double>(corr), d.n, ptr<double>(H), ptr<int32_t>(S), d.h, d.batch, thr, ptr<int32_t>(cnt),
                            ptr<double>(s1), ptr<double>(s2), current_stream()),
       "sfm_homography_score");
    return {cnt, s1, s2};
}

Tensor homography_inlier_mask_new(bool meta, const Tensor& corr, const Tensor& H, const Tensor& S, const Tensor& result, double thr) {
    const OpDevice scope(corr, meta);
    TORCH_CHECK(corr.dim() == 3, "sfm_hip: corr must be [batch, n, 4]");
    Dims d{};
    if (!meta) {
        need(corr, "corr", at::kDouble);
        need(H, "H", at::kDouble);
        need(S, "S", at::kInt);
        need(result, "result", at::kLong);
        d = hypothesis_dims(corr, S);
        check_H(H, d);
        TORCH_CHECK(result.numel() == d.batch * kRecordWords, "sfm_hip: result must be int64 [batch, 5]");
    }
    Tensor mask = alloc(corr, at::kByte, {corr.sym_size(0), corr.sym_size(1)});
    if (!meta)
        ok(sfm_homography_inlier_mask(ptr<double>(corr), d.n, ptr<double>(H), ptr<int32_t>(S), d.h, d.batch,
                                      reinterpret_cast<const sfm_select_result*>(ptr<int64_t>(result)), thr, ptr<uint8_t>(mask),
                                      current_stream()),
           "sfm_homography_inlier_mask");
    return mask;
}

// the whole homography pass (sfm_homography_ransac_pass): the arguments of five_point_ransac_pass_ with H for E
void homography_ransac_pass_out(const Tensor& corr, int64_t seed, int64_t seed_stride, bool use_philox, int64_t h_begin, double thr,
                                double min_extra, int64_t aggregation, Tensor& S, Tensor& H, Tensor& flags, Tensor& cnt, Tensor& s1,
                                Tensor& s2, Tensor& result, const std::optional<Tensor>& mask) {
    const OpDevice scope(corr);
    const Dims d = pass_checks(corr, "corr", hypothesis_dims, S, H, "H", flags, cnt, s1, s2, result, mask);
    check_H(H, d);
    ok(sfm_homography_ransac_pass((uint64_t)seed, (uint64_t)seed_stride, use_philox ? 1 : 0, h_begin, ptr<double>(corr), d.n, d.h,
                                  d.batch, thr, min_extra, (int)aggregation, ptr<int32_t>(S), ptr<double>(H), ptr<int32_t>(flags),
                                  ptr<int32_t>(cnt), ptr<double>(s1), ptr<double>(s2),
                                  reinterpret_cast<sfm_select_result*>(ptr<int64_t>(result)), ptr<uint8_t>(mask), current_stream()),
       "sfm_homography_ransac_pass");
}


// ---- the ragged two-view pass over a match graph (sfm_view_graph.hip): corr [n_total, 4], offset int64 [pairs + 1], min_extra
// double [pairs]; S [pairs, h, 8], H / E [pairs, h, 9], the score tables [pairs, h], the records int64 [pairs, 5], the masks
// uint8 [n_total], verdict int64 [pairs, 3] (sfm_pair_verdict) ----------------------------------------------------------
void verify_pairs_out(const Tensor& corr, const Tensor& offset, const Tensor& min_extra, int64_t seed, int64_t seed_stride,
                      int64_t h_begin, double thr, int64_t aggregation, double max_ratio, Tensor& S, Tensor& H, Tensor& E,
                      Tensor& h_flags, Tensor& h_cnt, Tensor& h_s1, Tensor& h_s2, Tensor& e_flags, Tensor& e_cnt, Tensor& e_s1,
                      Tensor& e_s2, Tensor& h_result, Tensor& e_result, Tensor& h_mask, Tensor& e_mask, Tensor& verdict) {
    const OpDevice scope(corr);
    static_assert(sizeof(sfm_pair_verdict) == 24, "verdict rows are three int64");
    need(corr, "corr", at::kDouble);
    need(offset, "offset", at::kLong);
    need(min_extra, "min_extra", at::kDouble);
    need(S, "S", at::kInt);
    need(H, "H", at::kDouble);
    need(E, "E", at::kDouble);
    for (const Tensor* t : {&h_flags, &h_cnt, &e_flags, &e_cnt}) need(*t, "flags / cnt", at::kInt);
    for (const Tensor* t : {&h_s1, &h_s2, &e_s1, &e_s2}) need(*t, "s1 / s2", at::kDouble);
    for (const Tensor* t : {&h_result, &e_result, &verdict}) need(*t, "result / verdict", at::kLong);
    need(h_mask, "h_mask", at::kByte);
    need(e_mask, "e_mask", at::kByte);
    TORCH_CHECK(corr.dim() == 2 && corr.size(1) == 4, "sfm_hip: corr must be [n_total, 4]");
    TORCH_CHECK(offset.dim() == 1 && offset.size(0) >= 1, "sfm_hip: offset must be int64 [pairs + 1]");
    const int64_t n_total = corr.size(0), pairs = offset.size(0) - 1;
    TORCH_CHECK(S.dim() == 3 && S.size(0) == pairs && S.size(2) == 8, "sfm_hip: S must be [pairs, h, 8]");
    const int64_t h = S.size(1);
    TORCH_CHECK(min_extra.numel() == pairs, "sfm_hip: min_extra must be [pairs]");
    TORCH_CHECK(H.numel() == pairs * h * 9 && E.numel() == pairs * h * 9, "sfm_hip: H, E must be [pairs, h, 9]");
    for (const Tensor* t : {&h_flags, &h_cnt, &h_s1, &h_s2, &e_flags, &e_cnt, &e_s1, &e_s2})
        TORCH_CHECK(t->numel() == pairs * h, "sfm_hip: flags, cnt, s1, s2 must be [pairs, h]");
    TORCH_CHECK(h_result.numel() == pairs * kRecordWords && e_result.numel() == pairs * kRecordWords,
                "sfm_hip: h_result, e_result must be int64 [pairs, 5]");
    TORCH_CHECK(h_mask.numel() == n_total && e_mask.numel() == n_total, "sfm_hip: h_mask, e_mask must be uint8 [n_total]");
    TORCH_CHECK(verdict.numel() == pairs * 3, "sfm_hip: verdict must be int64 [pairs, 3]");
    ok(sfm_verify_pairs((uint64_t)seed, (uint64_t)seed_stride, h_begin, ptr<double>(corr), n_total, ptr<int64_t>(offset), pairs,
                        ptr<double>(min_extra), h, thr, (int)aggregation, max_ratio, ptr<int32_t>(S), ptr<double>(H), ptr<double>(E),
                        ptr<int32_t>(h_flags), ptr<int32_t>(h_cnt), ptr<double>(h_s1), ptr<double>(h_s2), ptr<int32_t>(e_flags),
                        ptr<int32_t>(e_cnt), ptr<double>(e_s1), ptr<double>(e_s2),
                        reinterpret_cast<sfm_select_result*>(ptr<int64_t>(h_result)),
                        reinterpret_cast<sfm_select_result*>(ptr<int64_t>(e_result)), ptr<uint8_t>(h_mask), ptr<uint8_t>(e_mask),
                        reinterpret_cast<sfm_pair_verdict*>(ptr<int64_t>(verdict)), current_stream()),
       "sfm_verify_pairs");
}

// ---- relative pose and triangulation angle of every pair behind verify_pairs_ (sfm_view_graph_pose.hip), on that op's tensors:
// -> (pose uint8 [pairs, 128], the sfm_pair_pose records; angle double [n_total], each item's angle under its pair's best pose,
// NaN off the passing inliers: the head of the call's workspace) ------------------------------------------------------------
// what the two ops behind verify_pairs_ check of corr and offset before they allocate -> n_total, pairs (0, 0 under Meta)
std::pair<int64_t, int64_t> ragged_pair_dims(bool meta, const Tensor& corr, const Tensor& offset) {
    if (meta) {
        TORCH_CHECK(corr.dim() == 2 && offset.dim() == 1, "sfm_hip: corr must be [n_total, 4], offset int64 [pairs + 1]");
        return {0, 0};
    }
    TORCH_CHECK(corr.dim() == 2 && corr.size(1) == 4, "sfm_hip: corr must be [n_total, 4]");
    TORCH_CHECK(offset.dim() == 1 && offset.size(0) >= 1, "sfm_hip: offset must be int64 [pairs + 1]");
    return {corr.size(0), offset.size(0) - 1};
}

std::tuple<Tensor, Tensor> pair_poses_new(bool meta, const Tensor& corr, const Tensor& offset, const Tensor& E, const Tensor& e_result,
                                          const Tensor& e_mask, const Tensor& verdict, double distance_threshold) {
    const OpDevice scope(corr, meta);
    static_assert(sizeof(sfm_pair_pose) == 128, "pose rows are 128 bytes");
    if (!meta) {
        need(corr, "corr", at::kDouble);
        need(offset, "offset", at::kLong);
        need(E, "E", at::kDouble);
        need(e_result, "e_result", at::kLong);
        need(e_mask, "e_mask", at::kByte);
        need(verdict, "verdict", at::kLong);
    }
    const auto [n_total, pairs] = ragged_pair_dims(meta, corr, offset);
    int64_t bytes = 0;
    if (!meta) {
        TORCH_CHECK(E.dim() == 3 && E.size(0) == pairs && E.size(1) >= 1 && E.size(2) == 9, "sfm_hip: E must be [pairs, h >= 1, 9]");
        TORCH_CHECK(e_result.numel() == pairs * kRecordWords, "sfm_hip: e_result must be int64 [pairs, 5]");
        TORCH_CHECK(e_mask.numel() == n_total, "sfm_hip: e_mask must be uint8 [n_total]");
        TORCH_CHECK(verdict.numel() == pairs * 3, "sfm_hip: verdict must be int64 [pairs, 3]");
        bytes = sfm_pair_poses_workspace_bytes(n_total, pairs);
        TORCH_CHECK(bytes >= 0, "sfm_hip: pair_poses takes at most 65535 pairs and fewer than 2^31 items");
    }
    Tensor pose = alloc(corr, at::kByte, {offset.sym_size(0) - 1, 128});
    if (meta) return {pose, alloc(corr, at::kDouble, {corr.sym_size(0)})};   // angle: on the device the head of the workspace
    Tensor workspace = at::empty({(bytes + 7) / 8}, like(corr, at::kDouble));
    if (pairs == 0) workspace.fill_(NAN);   // the entry is a no-op then: no item has a pair
    ok(sfm_pair_poses(ptr<double>(corr), n_total, ptr<int64_t>(offset), pairs, ptr<double>(E), E.size(1),
                      reinterpret_cast<const sfm_select_result*>(ptr<int64_t>(e_result)), ptr<uint8_t>(e_mask),
                      reinterpret_cast<const sfm_pair_verdict*>(ptr<int64_t>(verdict)), distance_threshold,
                      reinterpret_cast<sfm_pair_pose*>(ptr<uint8_t>(pose)), workspace.data_ptr(), bytes, current_stream()),
       "sfm_pair_poses");
    return {pose, workspace.narrow(0, 0, n_total)};
}

// ---- refinement of every pair's pose on its inliers behind pair_poses (sfm_view_graph_refine.hip): pose uint8 [pairs, 128] as
// pair_poses returned it -> (pose_out uint8 [pairs, 128]; mask uint8 [n_total], 1 = within thr under the kept pose; info int64
// [pairs, 5] viewing the sfm_pair_refine_info records) ------------------------------------------------------------------------
constexpr int64_t kPairRefineInfoWords = sizeof(sfm_pair_refine_info) / 8;

std::tuple<Tensor, Tensor, Tensor> refine_pair_poses_new(bool meta, const Tensor& corr, const Tensor& offset, const Tensor& pose,
                                                         double thr, int64_t aggregation, int64_t rounds, int64_t max_steps) {
    const OpDevice scope(corr, meta);
    static_assert(sizeof(sfm_pair_pose) == 128 && sizeof(sfm_pair_refine_info) == 40, "pose rows are 128 bytes, info rows 40");
    if (!meta) {
        need(corr, "corr", at::kDouble);
        need(offset, "offset", at::kLong);
        need(pose, "pose", at::kByte);
    }
    const auto [n_total, pairs] = ragged_pair_dims(meta, corr, offset);
    if (!meta) {
        TORCH_CHECK(pose.numel() == pairs * 128, "sfm_hip: pose must be uint8 [pairs, 128]");
        TORCH_CHECK(rounds >= 0 && rounds <= 0x7FFFFFFF && max_steps >= 0 && max_steps <= 0x7FFFFFFF,
                    "sfm_hip: rounds and max_steps must be in [0, 2^31)");
    }
    Tensor pose_out = alloc(corr, at::kByte, {offset.sym_size(0) - 1, 128});
    Tensor mask = alloc(corr, at::kByte, {corr.sym_size(0)});
    Tensor info = alloc(corr, at::kLong, {offset.sym_size(0) - 1, kPairRefineInfoWords});
    if (meta) return {pose_out, mask, info};
    if (pairs == 0) mask.zero_();   // the entry is a no-op then: no item has a pair
    ok(sfm_refine_pair_poses(ptr<double>(corr), n_total, ptr<int64_t>(offset), pairs,
                             reinterpret_cast<const sfm_pair_pose*>(ptr<uint8_t>(pose)), thr, (int)aggregation, (int)rounds,
                             (int)max_steps, reinterpret_cast<sfm_pair_pose*>(ptr<uint8_t>(pose_out)), ptr<uint8_t>(mask),
                             reinterpret_cast<sfm_pair_refine_info*>(ptr<int64_t>(info)), current_stream()),
       "sfm_refine_pair_poses");
    return {pose_out, mask, info};
}

// ---- PnP (sfm_pnp.hip): pts [batch, n, 5] = {X, Y, Z, u, v}, K 9 doubles (row-major, row 2 = 0 0 1), S [batch, h, 8],
// model [batch, h, 12] = R (9) | t (3) ----------------------------------------------------------------------------------
Dims pnp_dims(const Tensor& pts, const Tensor& S) {
    TORCH_CHECK(pts.dim() == 3 && pts.size(2) == 5, "sfm_hip: pts must be [batch, n, 5]");
    TORCH_CHECK(S.dim() == 3 && S.size(0) == pts.size(0) && S.size(2) == 8, "sfm_hip: S must be [batch, h, 8]");
    return {pts.size(0), pts.size(1), S.size(1)};
}

// what a functional form over pts and S checks before it allocates: under Meta the ranks alone, in words of its own
void pose_dims(bool meta, const Tensor& pts, const Tensor& S) {
    if (meta) {
        TORCH_CHECK(pts.dim() == 3 && S.dim() == 3, "sfm_hip: pts [batch, n, 5], S [batch, h, 8]");
    } else {
        pnp_dims(pts, S);
    }
}

void check_K(at::ArrayRef<double> K) { TORCH_CHECK(K.size() == 9, "sfm_hip: K must hold 9 doubles (3 x 3, row-major)"); }

void check_model(const Tensor& model, const Dims& d) {
    TORCH_CHECK(model.dim() == 3 && model.size(0) == d.batch && model.size(1) == d.h && model.size(2) == 12,
                "sfm_hip: model must be [batch, h, 12]");
}

// pnp_fit (six-point DLT) and p3p_fit (four-item samples, sfm_p3p.h): one body, the entry point differs
using PoseFit = int (*)(const double*, int64_t, const int32_t*, int64_t, int64_t, const double*, double*, int32_t*, void*);

void pose_fit(PoseFit entry, const char* name, const Tensor& pts, const Tensor& S, at::ArrayRef<double> K, Tensor& model,
              Tensor& flags) {
    const OpDevice scope(pts);
    need(pts, "pts", at::kDouble);
    need(S, "S", at::kInt);
    need(model, "model", at::kDouble);
    need(flags, "flags", at::kInt);
    check_K(K);
    const Dims d = pnp_dims(pts, S);
    check_model(model, d);
    TORCH_CHECK(flags.numel() == d.batch * d.h, "sfm_hip: flags must be [batch, h]");
    ok(entry(ptr<double>(pts), d.n, ptr<int32_t>(S), d.h, d.batch, K.data(), ptr<double>(model), ptr<int32_t>(flags), current_stream()),
       name);
}

void pnp_fit_out(const Tensor& pts, const Tensor& S, at::ArrayRef<double> K, Tensor& model, Tensor& flags) {
    pose_fit(sfm_pnp_fit, "sfm_pnp_fit", pts, S, K, model, flags);
}

void p3p_fit_out(const Tensor& pts, const Tensor& S, at::ArrayRef<double> K, Tensor& model, Tensor& flags) {
    pose_fit(sfm_p3p_fit, "sfm_p3p_fit", pts, S, K, model, flags);
}

template <void (*FitOut)(const Tensor&, const Tensor&, at::ArrayRef<double>, Tensor&, Tensor&)>
std::tuple<Tensor, Tensor> pose_fit_new(bool meta, const Tensor& pts, const Tensor& S, at::ArrayRef<double> K) {
    pose_dims(meta, pts, S);
    Tensor model = alloc(pts, at::kDouble, {pts.sym_size(0), S.sym_size(1), 12});
    Tensor flags = alloc(pts, at::kInt, {pts.sym_size(0), S.sym_size(1)});
    if (!meta) FitOut(pts, S, K, model, flags);
    return {model, flags};
}

void pnp_score_out(const Tensor& pts, const Tensor& model, const Tensor& S, at::ArrayRef<double> K, double thr, Tensor& cnt,
                   Tensor& s1, Tensor& s2, int64_t sample_size) {
    const OpDevice scope(pts);
    need(pts, "pts", at::kDouble);
    need(model, "model", at::kDouble);
    need(S, "S", at::kInt);
    need(cnt, "cnt", at::kInt);
    need(s1, "s1", at::kDouble);
    need(s2, "s2", at::kDouble);
    check_K(K);
    const Dims d = pnp_dims(pts, S);
    check_model(model, d);
    TORCH_CHECK(cnt.numel() == d.batch * d.h && s1.numel() == d.batch * d.h && s2.numel() == d.batch * d.h,
                "sfm_hip: cnt, s1, s2 must be [batch, h]");
    ok(sfm_pnp_score(ptr<double>(pts), d.n, ptr<double>(model), ptr<int32_t>(S), d.h, d.batch, K.data(), thr, (int)sample_size,
                     ptr<int32_t>(cnt), ptr<double>(s1), ptr<double>(s2), current_stream()),
       "sfm_pnp_score");
}

std::tuple<Tensor, Tensor, Tensor> pnp_score_new(bool meta, const Tensor& pts, const Tensor& model, const Tensor& S,
                                                 at::ArrayRef<double> K, double thr, int64_t sample_size) {
    pose_dims(meta, pts, S);
    const SymInt b = pts.sym_size(0), h = S.sym_size(1);
    Tensor cnt = alloc(pts, at::kInt, {b, h}), s1 = alloc(pts, at::kDouble, {b, h}), s2 = alloc(pts, at::kDouble, {b, h});
    if (!meta) pnp_score_out(pts, model, S, K, thr, cnt, s1, s2, sample_size);
    return {cnt, s1, s2};
}

// the whole pass of `solver` into the caller's buffers (device.PnPWorkspace); `mask` optional
void pnp_pass(int solver, const Tensor& pts, int64_t seed, int64_t seed_stride, bool use_philox, int64_t h_begin,
              at::ArrayRef<double> K, double thr, double min_extra, int64_t aggregation, Tensor& S, Tensor& model, Tensor& flags,
              Tensor& cnt, Tensor& s1, Tensor& s2, Tensor& result, const std::optional<Tensor>& mask) {
    const OpDevice scope(pts);
    check_K(K);
    const Dims d = pass_checks(pts, "pts", pnp_dims, S, model, "model", flags, cnt, s1, s2, result, mask);
    check_model(model, d);
    ok(sfm_pnp_ransac_pass(solver, (uint64_t)seed, (uint64_t)seed_stride, use_philox ? 1 : 0, h_begin, ptr<double>(pts), d.n, d.h,
                           d.batch, K.data(), thr, min_extra, (int)aggregation, ptr<int32_t>(S), ptr<double>(model),
                           ptr<int32_t>(flags), ptr<int32_t>(cnt), ptr<double>(s1), ptr<double>(s2),
                           reinterpret_cast<sfm_select_result*>(ptr<int64_t>(result)), ptr<uint8_t>(mask), current_stream()),
       "sfm_pnp_ransac_pass");
}

void pnp_ransac_pass_out(const Tensor& pts, int64_t seed, int64_t seed_stride, bool use_philox, int64_t h_begin,
                         at::ArrayRef<double> K, double thr, double min_extra, int64_t aggregation, Tensor& S, Tensor& model,
                         Tensor& flags, Tensor& cnt, Tensor& s1, Tensor& s2, Tensor& result, const std::optional<Tensor>& mask) {
    pnp_pass(SFM_PNP_SOLVER_DLT, pts, seed, seed_stride, use_philox, h_begin, K, thr, min_extra, aggregation, S, model, flags, cnt, s1,
             s2, result, mask);
}

// the P3P pass: the arguments of pnp_ransac_pass_
void p3p_ransac_pass_out(const Tensor& pts, int64_t seed, int64_t seed_stride, bool use_philox, int64_t h_begin,
                         at::ArrayRef<double> K, double thr, double min_extra, int64_t aggregation, Tensor& S, Tensor& model,
                         Tensor& flags, Tensor& cnt, Tensor& s1, Tensor& s2, Tensor& result, const std::optional<Tensor>& mask) {
    pnp_pass(SFM_PNP_SOLVER_P3P, pts, seed, seed_stride, use_philox, h_begin, K, thr, min_extra, aggregation, S, model, flags, cnt, s1,
             s2, result, mask);
}

// refinement of a winner on its inliers (sfm_pnp_refine.hip): model [batch, 12], mask uint8 [batch, n], err [batch];
// info int64 [batch, 3] viewing the sfm_pnp_refine_info records
constexpr int64_t kRefineInfoWords = sizeof(sfm_pnp_refine_info) / 8;

void pnp_refine_out(const Tensor& pts, const Tensor& model, const Tensor& mask, const Tensor& err, at::ArrayRef<double> K,
                    double thr, int64_t aggregation, int64_t rounds, int64_t max_steps, Tensor& model_out, Tensor& mask_out,
                    Tensor& info) {
    const OpDevice scope(pts);
    need(pts, "pts", at::kDouble);
    need(model, "model", at::kDouble);
    need(mask, "mask", at::kByte);
    need(err, "err", at::kDouble);
    need(model_out, "model_out", at::kDouble);
    need(mask_out, "mask_out", at::kByte);
    need(info, "info", at::kLong);
    check_K(K);
    TORCH_CHECK(pts.dim() == 3 && pts.size(2) == 5, "sfm_hip: pts must be [batch, n, 5]");
    const int64_t batch = pts.size(0), n = pts.size(1);
    TORCH_CHECK(model.numel() == batch * 12 && model_out.numel() == batch * 12, "sfm_hip: model, model_out must be [batch, 12]");
    TORCH_CHECK(mask.numel() == batch * n && mask_out.numel() == batch * n, "sfm_hip: mask, mask_out must be uint8 [batch, n]");
    TORCH_CHECK(err.numel() == batch, "sfm_hip: err must be [batch]");
    TORCH_CHECK(info.numel() == batch * kRefineInfoWords, "sfm_hip: info must be int64 [batch, 3]");
    ok(sfm_pnp_refine(ptr<double>(pts), n, batch, K.data(), ptr<double>(model), ptr<uint8_t>(mask), ptr<double>(err), thr,
                      (int)aggregation, (int)rounds, (int)max_steps, ptr<double>(model_out), ptr<uint8_t>(mask_out),
                      reinterpret_cast<sfm_pnp_refine_info*>(ptr<int64_t>(info)), current_stream()),
       "sfm_pnp_refine");
}

std::tuple<Tensor, Tensor, Tensor> pnp_refine_new(bool meta, const Tensor& pts, const Tensor& model, const Tensor& mask,
                                                  const Tensor& err, at::ArrayRef<double> K, double thr, int64_t aggregation,
                                                  int64_t rounds, int64_t max_steps) {
    TORCH_CHECK(pts.dim() == 3, "sfm_hip: pts must be [batch, n, 5]");
    Tensor model_out = alloc(pts, at::kDouble, {pts.sym_size(0), 12});
    Tensor mask_out = alloc(pts, at::kByte, {pts.sym_size(0), pts.sym_size(1)});
    Tensor info = alloc(pts, at::kLong, {pts.sym_size(0), kRefineInfoWords});
    if (!meta) pnp_refine_out(pts, model, mask, err, K, thr, aggregation, rounds, max_steps, model_out, mask_out, info);
    return {model_out, mask_out, info};
}

// ---- absolute pose of every candidate view in one call (sfm_register_views.hip): pts [n_total, 5], offset int64 [views + 1],
// min_extra double [views]; S [views, h, 8], model [views, h, 12], the score tables [views, h], result int64 [views, 5], mask
// uint8 [n_total]; pose_out [views, 12], mask_out uint8 [n_total], info int64 [views, 3] (sfm_pnp_refine_info), status int32
// [views] ------------------------------------------------------------------------------------------------------------------
void register_views_out(const Tensor& pts, const Tensor& offset, const Tensor& min_extra, at::ArrayRef<double> K, int64_t seed,
                        int64_t seed_stride, int64_t h_begin, double thr, int64_t aggregation, int64_t refine_rounds,
                        int64_t refine_max_steps, Tensor& S, Tensor& model, Tensor& flags, Tensor& cnt, Tensor& s1, Tensor& s2,
                        Tensor& result, Tensor& mask, Tensor& pose_out, Tensor& mask_out, Tensor& info, Tensor& status) {
    const OpDevice scope(pts);
    need(pts, "pts", at::kDouble);
    need(offset, "offset", at::kLong);
    need(min_extra, "min_extra", at::kDouble);
    need(S, "S", at::kInt);
    need(model, "model", at::kDouble);
    for (const Tensor* t : {&flags, &cnt, &status}) need(*t, "flags / cnt / status", at::kInt);
    for (const Tensor* t : {&s1, &s2, &pose_out}) need(*t, "s1 / s2 / pose_out", at::kDouble);
    for (const Tensor* t : {&result, &info}) need(*t, "result / info", at::kLong);
    need(mask, "mask", at::kByte);
    need(mask_out, "mask_out", at::kByte);
    check_K(K);
    TORCH_CHECK(pts.dim() == 2 && pts.size(1) == 5, "sfm_hip: pts must be [n_total, 5]");
    TORCH_CHECK(offset.dim() == 1 && offset.size(0) >= 1, "sfm_hip: offset must be int64 [views + 1]");
    const int64_t n_total = pts.size(0), views = offset.size(0) - 1;
    TORCH_CHECK(S.dim() == 3 && S.size(0) == views && S.size(2) == 8, "sfm_hip: S must be [views, h, 8]");
    const int64_t h = S.size(1);
    TORCH_CHECK(min_extra.numel() == views, "sfm_hip: min_extra must be [views]");
    TORCH_CHECK(model.numel() == views * h * 12, "sfm_hip: model must be [views, h, 12]");
    for (const Tensor* t : {&flags, &cnt, &s1, &s2}) TORCH_CHECK(t->numel() == views * h, "sfm_hip: flags, cnt, s1, s2 must be [views, h]");
    TORCH_CHECK(result.numel() == views * kRecordWords, "sfm_hip: result must be int64 [views, 5]");
    TORCH_CHECK(mask.numel() == n_total && mask_out.numel() == n_total, "sfm_hip: mask, mask_out must be uint8 [n_total]");
    TORCH_CHECK(pose_out.numel() == views * 12, "sfm_hip: pose_out must be [views, 12]");
    TORCH_CHECK(info.numel() == views * kRefineInfoWords, "sfm_hip: info must be int64 [views, 3]");
    TORCH_CHECK(status.numel() == views, "sfm_hip: status must be int32 [views]");
    TORCH_CHECK(refine_rounds >= 0 && refine_rounds <= 0x7FFFFFFF && refine_max_steps >= 0 && refine_max_steps <= 0x7FFFFFFF,
                "sfm_hip: refine_rounds and refine_max_steps must be in [0, 2^31)");
    ok(sfm_register_views((uint64_t)seed, (uint64_t)seed_stride, h_begin, ptr<double>(pts), n_total, ptr<int64_t>(offset), views,
                          ptr<double>(min_extra), K.data(), h, thr, (int)aggregation, (int)refine_rounds, (int)refine_max_steps,
                          ptr<int32_t>(S), ptr<double>(model), ptr<int32_t>(flags), ptr<int32_t>(cnt), ptr<double>(s1), ptr<double>(s2),
                          reinterpret_cast<sfm_select_result*>(ptr<int64_t>(result)), ptr<uint8_t>(mask), ptr<double>(pose_out),
                          ptr<uint8_t>(mask_out), reinterpret_cast<sfm_pnp_refine_info*>(ptr<int64_t>(info)), ptr<int32_t>(status),
                          current_stream()),
       "sfm_register_views");
}

// the functional form: h hypotheses per view -> (pose_out, mask_out, info, status, mask, result); the tables of the pass are
// temporaries of the call
// The tables of a ragged pass over `rows` groups with h hypotheses each, temporaries of a functional call: S, model [rows, h,
// width], flags, cnt, s1, s2
struct PassTables {
    Tensor S, model, flags, cnt, s1, s2;
    PassTables(const Tensor& t, const SymInt& rows, int64_t h, int64_t width)
        : S(alloc(t, at::kInt, {rows, h, 8})), model(alloc(t, at::kDouble, {rows, h, width})), flags(alloc(t, at::kInt, {rows, h})),
          cnt(alloc(t, at::kInt, {rows, h})), s1(alloc(t, at::kDouble, {rows, h})), s2(alloc(t, at::kDouble, {rows, h})) {}
};

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> register_views_new(bool meta, const Tensor& pts, const Tensor& offset,
                                                                              const Tensor& min_extra, at::ArrayRef<double> K,
                                                                              int64_t seed, int64_t seed_stride, int64_t h_begin,
                                                                              int64_t h, double thr, int64_t aggregation,
                                                                              int64_t refine_rounds, int64_t refine_max_steps) {
    TORCH_CHECK(pts.dim() == 2 && offset.dim() == 1 && (meta || offset.size(0) >= 1),
                "sfm_hip: pts must be [n_total, 5], offset int64 [views + 1]");
    if (!meta) TORCH_CHECK(h >= 1, "sfm_hip: register_views needs at least one hypothesis per view");
    const SymInt n_total = pts.sym_size(0), views = offset.sym_size(0) - 1;
    std::optional<PassTables> pass;
    if (!meta) pass.emplace(pts, views, h, 12);
    Tensor result = alloc(pts, at::kLong, {views, kRecordWords});
    Tensor mask = alloc(pts, at::kByte, {n_total}), mask_out = alloc(pts, at::kByte, {n_total});
    Tensor pose_out = alloc(pts, at::kDouble, {views, 12});
    Tensor info = alloc(pts, at::kLong, {views, kRefineInfoWords});
    Tensor status = alloc(pts, at::kInt, {views});
    if (!meta) {
        if (offset.size(0) == 1) {   // the entry is a no-op then: no item has a view
            mask.zero_();
            mask_out.zero_();
        }
        register_views_out(pts, offset, min_extra, K, seed, seed_stride, h_begin, thr, aggregation, refine_rounds, refine_max_steps, pass->S,
                           pass->model, pass->flags, pass->cnt, pass->s1, pass->s2, result, mask, pose_out, mask_out, info, status);
    }
    return {pose_out, mask_out, info, status, mask, result};
}

// ---- similarity alignment of two reconstructions (sfm_similarity.hip): pairs [batch, n, 6], S [batch, h, 8] (first 3 entries
// used), model [batch, h, 13] = R | t | s; the masked fit and the refinement take model [batch, 13], mask uint8 [batch, n], err
// [batch] and leave info int64 [batch, 3] viewing the sfm_similarity_refine_info records.  Their workspaces come from the
// caching allocator, stream-ordered like everything else ----------------------------------------------------------------
constexpr int64_t kSimilarityModelWidth = 13;
constexpr int64_t kSimilarityInfoWords = sizeof(sfm_similarity_refine_info) / 8;

Dims similarity_dims(const Tensor& pairs, const Tensor& S) {
    TORCH_CHECK(pairs.dim() == 3 && pairs.size(2) == 6, "sfm_hip: pairs must be [batch, n, 6]");
    TORCH_CHECK(S.dim() == 3 && S.size(0) == pairs.size(0) && S.size(2) == 8, "sfm_hip: S must be [batch, h, 8]");
    return {pairs.size(0), pairs.size(1), S.size(1)};
}

void similarity_ransac_pass_out(const Tensor& pairs, int64_t seed, int64_t seed_stride, bool use_philox, int64_t h_begin, double thr,
                                double min_extra, int64_t aggregation, Tensor& S, Tensor& model, Tensor& flags, Tensor& cnt, Tensor& s1,
                                Tensor& s2, Tensor& result, const std::optional<Tensor>& mask) {
    const OpDevice scope(pairs);
    const Dims d = pass_checks(pairs, "pairs", similarity_dims, S, model, "model", flags, cnt, s1, s2, result, mask);
    TORCH_CHECK(model.dim() == 3 && model.size(0) == d.batch && model.size(1) == d.h && model.size(2) == kSimilarityModelWidth,
                "sfm_hip: model must be [batch, h, 13]");
    ok(sfm_similarity_ransac_pass((uint64_t)seed, (uint64_t)seed_stride, use_philox ? 1 : 0, h_begin, ptr<double>(pairs), d.n, d.h,
                                  d.batch, thr, min_extra, (int)aggregation, ptr<int32_t>(S), ptr<double>(model), ptr<int32_t>(flags),
                                  ptr<int32_t>(cnt), ptr<double>(s1), ptr<double>(s2),
                                  reinterpret_cast<sfm_select_result*>(ptr<int64_t>(result)), ptr<uint8_t>(mask), current_stream()),
       "sfm_similarity_ransac_pass");
}

// the functional form: h Philox-sampled hypotheses per entry -> (model, flags, cnt, s1, s2, S, result, mask)
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> similarity_ransac_pass_new(bool meta, const Tensor& pairs,
                                                                                                      int64_t seed, int64_t seed_stride,
                                                                                                      int64_t h_begin, int64_t h, double thr,
                                                                                                      double min_extra,
                                                                                                      int64_t aggregation) {
    TORCH_CHECK(pairs.dim() == 3, "sfm_hip: pairs must be [batch, n, 6]");
    if (!meta) TORCH_CHECK(h >= 0, "sfm_hip: similarity_ransac_pass needs h >= 0");
    PassTables t(pairs, pairs.sym_size(0), h, kSimilarityModelWidth);
    Tensor result = alloc(pairs, at::kLong, {pairs.sym_size(0), kRecordWords});
    Tensor mask = alloc(pairs, at::kByte, {pairs.sym_size(0), pairs.sym_size(1)});
    if (!meta)
        similarity_ransac_pass_out(pairs, seed, seed_stride, true, h_begin, thr, min_extra, aggregation, t.S, t.model, t.flags, t.cnt, t.s1,
                                   t.s2, result, mask);
    return {t.model, t.flags, t.cnt, t.s1, t.s2, t.S, result, mask};
}

Tensor similarity_workspace(const Tensor& pairs, int64_t bytes, const char* what) {
    TORCH_CHECK(bytes >= 0, "sfm_hip: ", what, " refuses these sizes (need 3 <= n < 2^31 and batch <= 65535)");
    return at::empty({bytes > 16 ? bytes : 16}, like(pairs, at::kByte));
}

void similarity_fit_out(const Tensor& pairs, const std::optional<Tensor>& mask, Tensor& model_out, Tensor& flags_out) {
    const OpDevice scope(pairs);
    need(pairs, "pairs", at::kDouble);
    if (mask.has_value()) need(*mask, "mask", at::kByte);
    need(model_out, "model_out", at::kDouble);
    need(flags_out, "flags_out", at::kInt);
    TORCH_CHECK(pairs.dim() == 3 && pairs.size(2) == 6, "sfm_hip: pairs must be [batch, n, 6]");
    const int64_t batch = pairs.size(0), n = pairs.size(1);
    TORCH_CHECK(!mask.has_value() || mask->numel() == batch * n, "sfm_hip: mask must be uint8 [batch, n]");
    TORCH_CHECK(model_out.numel() == batch * kSimilarityModelWidth, "sfm_hip: model_out must be [batch, 13]");
    TORCH_CHECK(flags_out.numel() == batch, "sfm_hip: flags_out must be int32 [batch]");
    Tensor ws = similarity_workspace(pairs, sfm_similarity_fit_workspace_bytes(n, batch), "sfm_similarity_fit_masked");
    ok(sfm_similarity_fit_masked(ptr<double>(pairs), n, batch, ptr<uint8_t>(mask), ptr<double>(model_out), ptr<int32_t>(flags_out),
                                 ws.data_ptr(), ws.numel(), current_stream()),
       "sfm_similarity_fit_masked");
}

std::tuple<Tensor, Tensor> similarity_fit_new(bool meta, const Tensor& pairs, const std::optional<Tensor>& mask) {
    TORCH_CHECK(pairs.dim() == 3, "sfm_hip: pairs must be [batch, n, 6]");
    Tensor model_out = alloc(pairs, at::kDouble, {pairs.sym_size(0), kSimilarityModelWidth});
    Tensor flags_out = alloc(pairs, at::kInt, {pairs.sym_size(0)});
    if (!meta) similarity_fit_out(pairs, mask, model_out, flags_out);
    return {model_out, flags_out};
}

void similarity_refine_out(const Tensor& pairs, const Tensor& model, const Tensor& mask, const Tensor& err, double thr,
                           int64_t aggregation, int64_t rounds, Tensor& model_out, Tensor& mask_out, Tensor& info) {
    const OpDevice scope(pairs);
    need(pairs, "pairs", at::kDouble);
    need(model, "model", at::kDouble);
    need(mask, "mask", at::kByte);
    need(err, "err", at::kDouble);
    need(model_out, "model_out", at::kDouble);
    need(mask_out, "mask_out", at::kByte);
    need(info, "info", at::kLong);
    TORCH_CHECK(pairs.dim() == 3 && pairs.size(2) == 6, "sfm_hip: pairs must be [batch, n, 6]");
    const int64_t batch = pairs.size(0), n = pairs.size(1);
    TORCH_CHECK(model.numel() == batch * kSimilarityModelWidth && model_out.numel() == batch * kSimilarityModelWidth,
                "sfm_hip: model, model_out must be [batch, 13]");
    TORCH_CHECK(mask.numel() == batch * n && mask_out.numel() == batch * n, "sfm_hip: mask, mask_out must be uint8 [batch, n]");
    TORCH_CHECK(err.numel() == batch, "sfm_hip: err must be [batch]");
    TORCH_CHECK(info.numel() == batch * kSimilarityInfoWords, "sfm_hip: info must be int64 [batch, 3]");
    Tensor ws = similarity_workspace(pairs, sfm_similarity_refine_workspace_bytes(n, batch), "sfm_similarity_refine");
    ok(sfm_similarity_refine(ptr<double>(pairs), n, batch, ptr<double>(model), ptr<uint8_t>(mask), ptr<double>(err), thr,
                             (int)aggregation, (int)rounds, ptr<double>(model_out), ptr<uint8_t>(mask_out),
                             reinterpret_cast<sfm_similarity_refine_info*>(ptr<int64_t>(info)), ws.data_ptr(), ws.numel(),
                             current_stream()),
       "sfm_similarity_refine");
}

std::tuple<Tensor, Tensor, Tensor> similarity_refine_new(bool meta, const Tensor& pairs, const Tensor& model, const Tensor& mask,
                                                         const Tensor& err, double thr, int64_t aggregation, int64_t rounds) {
    TORCH_CHECK(pairs.dim() == 3, "sfm_hip: pairs must be [batch, n, 6]");
    Tensor model_out = alloc(pairs, at::kDouble, {pairs.sym_size(0), kSimilarityModelWidth});
    Tensor mask_out = alloc(pairs, at::kByte, {pairs.sym_size(0), pairs.sym_size(1)});
    Tensor info = alloc(pairs, at::kLong, {pairs.sym_size(0), kSimilarityInfoWords});
    if (!meta) similarity_refine_out(pairs, model, mask, err, thr, aggregation, rounds, model_out, mask_out, info);
    return {model_out, mask_out, info};
}

// ---- similarity alignment of every pair of sub-models in one call (sfm_align_models.hip): pairs [n_total, 6], offset int64
// [Q + 1], thr and min_extra double [Q]; S [Q, h, 8], model [Q, h, 13], the score tables [Q, h], result int64 [Q, 5], mask uint8
// [n_total]; model_out [Q, 13], mask_out uint8 [n_total], info int64 [Q, 3] (sfm_similarity_refine_info), status int32 [Q].
// max_items: an upper bound on every pair's item count.  The workspace comes from the caching allocator -------------------------
void align_models_out(const Tensor& pairs, const Tensor& offset, const Tensor& thr, const Tensor& min_extra, int64_t max_items,
                      int64_t seed, int64_t seed_stride, int64_t h_begin, int64_t aggregation, int64_t refine_rounds, Tensor& S,
                      Tensor& model, Tensor& flags, Tensor& cnt, Tensor& s1, Tensor& s2, Tensor& result, Tensor& mask, Tensor& model_out,
                      Tensor& mask_out, Tensor& info, Tensor& status) {
    const OpDevice scope(pairs);
    need(pairs, "pairs", at::kDouble);
    need(offset, "offset", at::kLong);
    need(thr, "thr", at::kDouble);
    need(min_extra, "min_extra", at::kDouble);
    need(S, "S", at::kInt);
    need(model, "model", at::kDouble);
    for (const Tensor* t : {&flags, &cnt, &status}) need(*t, "flags / cnt / status", at::kInt);
    for (const Tensor* t : {&s1, &s2, &model_out}) need(*t, "s1 / s2 / model_out", at::kDouble);
    for (const Tensor* t : {&result, &info}) need(*t, "result / info", at::kLong);
    need(mask, "mask", at::kByte);
    need(mask_out, "mask_out", at::kByte);
    TORCH_CHECK(pairs.dim() == 2 && pairs.size(1) == 6, "sfm_hip: pairs must be [n_total, 6]");
    TORCH_CHECK(offset.dim() == 1 && offset.size(0) >= 1, "sfm_hip: offset must be int64 [pairs + 1]");
    const int64_t n_total = pairs.size(0), Q = offset.size(0) - 1;
    TORCH_CHECK(S.dim() == 3 && S.size(0) == Q && S.size(2) == 8, "sfm_hip: S must be [pairs, h, 8]");
    const int64_t h = S.size(1);
    TORCH_CHECK(thr.numel() == Q && min_extra.numel() == Q, "sfm_hip: thr, min_extra must be [pairs]");
    TORCH_CHECK(model.numel() == Q * h * kSimilarityModelWidth, "sfm_hip: model must be [pairs, h, 13]");
    for (const Tensor* t : {&flags, &cnt, &s1, &s2}) TORCH_CHECK(t->numel() == Q * h, "sfm_hip: flags, cnt, s1, s2 must be [pairs, h]");
    TORCH_CHECK(result.numel() == Q * kRecordWords, "sfm_hip: result must be int64 [pairs, 5]");
    TORCH_CHECK(mask.numel() == n_total && mask_out.numel() == n_total, "sfm_hip: mask, mask_out must be uint8 [n_total]");
    TORCH_CHECK(model_out.numel() == Q * kSimilarityModelWidth, "sfm_hip: model_out must be [pairs, 13]");
    TORCH_CHECK(info.numel() == Q * kSimilarityInfoWords, "sfm_hip: info must be int64 [pairs, 3]");
    TORCH_CHECK(status.numel() == Q, "sfm_hip: status must be int32 [pairs]");
    TORCH_CHECK(refine_rounds >= 0 && refine_rounds <= 0x7FFFFFFF, "sfm_hip: refine_rounds must be in [0, 2^31)");
    const int64_t bytes = sfm_align_models_workspace_bytes(n_total, Q, max_items);
    TORCH_CHECK(bytes >= 0, "sfm_hip: sfm_align_models refuses these sizes (need n_total < 2^31, pairs <= 65535 and 0 <= max_items <= "
                            "n_total)");
    Tensor ws = at::empty({bytes > 16 ? bytes : 16}, like(pairs, at::kByte));
    ok(sfm_align_models((uint64_t)seed, (uint64_t)seed_stride, h_begin, ptr<double>(pairs), n_total, ptr<int64_t>(offset), Q, max_items,
                        ptr<double>(thr), ptr<double>(min_extra), h, (int)aggregation, (int)refine_rounds, ptr<int32_t>(S),
                        ptr<double>(model), ptr<int32_t>(flags), ptr<int32_t>(cnt), ptr<double>(s1), ptr<double>(s2),
                        reinterpret_cast<sfm_select_result*>(ptr<int64_t>(result)), ptr<uint8_t>(mask), ptr<double>(model_out),
                        ptr<uint8_t>(mask_out), reinterpret_cast<sfm_similarity_refine_info*>(ptr<int64_t>(info)), ptr<int32_t>(status),
                        ws.data_ptr(), ws.numel(), current_stream()),
       "sfm_align_models");
}

// the functional form: h hypotheses per pair -> (model_out, mask_out, info, status, mask, result); the tables of the pass are
// temporaries of the call
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> align_models_new(bool meta, const Tensor& pairs, const Tensor& offset,
                                                                            const Tensor& thr, const Tensor& min_extra, int64_t max_items,
                                                                            int64_t seed, int64_t seed_stride, int64_t h_begin, int64_t h,
                                                                            int64_t aggregation, int64_t refine_rounds) {
    TORCH_CHECK(pairs.dim() == 2 && offset.dim() == 1 && (meta || offset.size(0) >= 1),
                "sfm_hip: pairs must be [n_total, 6], offset int64 [pairs + 1]");
    if (!meta) TORCH_CHECK(h >= 1, "sfm_hip: align_models needs at least one hypothesis per pair");
    const SymInt n_total = pairs.sym_size(0), Q = offset.sym_size(0) - 1;
    std::optional<PassTables> pass;
    if (!meta) pass.emplace(pairs, Q, h, kSimilarityModelWidth);
    Tensor result = alloc(pairs, at::kLong, {Q, kRecordWords});
    Tensor mask = alloc(pairs, at::kByte, {n_total}), mask_out = alloc(pairs, at::kByte, {n_total});
    Tensor model_out = alloc(pairs, at::kDouble, {Q, kSimilarityModelWidth});
    Tensor info = alloc(pairs, at::kLong, {Q, kSimilarityInfoWords});
    Tensor status = alloc(pairs, at::kInt, {Q});
    if (!meta) {
        if (offset.size(0) == 1) {   // the entry is a no-op then: no item has a pair
            mask.zero_();
            mask_out.zero_();
        }
        align_models_out(pairs, offset, thr, min_extra, max_items, seed, seed_stride, h_begin, aggregation, refine_rounds, pass->S,
                         pass->model, pass->flags, pass->cnt, pass->s1, pass->s2, result, mask, model_out, mask_out, info, status);
    }
    return {model_out, mask_out, info, status, mask, result};
}

// ---- plane-sweep depth maps and their consistency filter (sfm_plane_sweep.hip): images uint8 [V, H, W], K [9] and poses [V, 12]
// on the device, refs int32 [R], sources int32 [R, S], depths [R, D]; depth, cost [R, H, W], index int32 [R, H, W], status int32 [R],
// volume [R, D, H, W] or none.  The workspace comes from the caching allocator ------------------------------------------------------
struct SweepDims {
    int64_t V, H, W, R, S, D;
};

SweepDims sweep_dims(const Tensor& maps, const Tensor& K, const Tensor& poses, const Tensor& refs, const Tensor& sources) {
    TORCH_CHECK(maps.dim() == 3, "sfm_hip: images / depth must be [views, height, width]");
    TORCH_CHECK(K.numel() == 9, "sfm_hip: K must hold 9 doubles");
    TORCH_CHECK(poses.dim() == 2 && poses.size(0) == maps.size(0) && poses.size(1) == 12, "sfm_hip: poses must be [views, 12]");
    TORCH_CHECK(refs.dim() == 1, "sfm_hip: refs must be int32 [refs]");
    TORCH_CHECK(sources.dim() == 2 && sources.size(0) == refs.size(0), "sfm_hip: sources must be int32 [refs, sources]");
    return {maps.size(0), maps.size(1), maps.size(2), refs.size(0), sources.size(1), 0};
}

void plane_sweep_out(const Tensor& images, const Tensor& K, const Tensor& poses, const Tensor& refs, const Tensor& sources,
                     const Tensor& depths, int64_t radius, int64_t top_k, int64_t min_sources, double min_variance, Tensor& depth,
                     Tensor& index, Tensor& cost, Tensor& status, const std::optional<Tensor>& volume) {
    const OpDevice scope(images);
    need(images, "images", at::kByte);
    for (const Tensor* t : {&K, &poses, &depths}) need(*t, "K / poses / depths", at::kDouble);
    for (const Tensor* t : {&depth, &cost}) need(*t, "depth / cost", at::kDouble);
    for (const Tensor* t : {&refs, &sources}) need(*t, "refs / sources", at::kInt);
    for (const Tensor* t : {&index, &status}) need(*t, "index / status", at::kInt);
    SweepDims d = sweep_dims(images, K, poses, refs, sources);
    TORCH_CHECK(depths.dim() == 2 && depths.size(0) == d.R, "sfm_hip: depths must be [refs, depths]");
    d.D = depths.size(1);
    const int64_t pixels = d.R * d.H * d.W;
    TORCH_CHECK(depth.numel() == pixels && cost.numel() == pixels && index.numel() == pixels,
                "sfm_hip: depth, index, cost must be [refs, height, width]");
    TORCH_CHECK(status.numel() == d.R, "sfm_hip: status must be int32 [refs]");
    const bool with_volume = volume.has_value() && volume->defined();
    if (with_volume) {
        need(*volume, "volume", at::kDouble);
        TORCH_CHECK(volume->numel() == pixels * d.D, "sfm_hip: volume must be [refs, depths, height, width]");
    }
    for (int64_t v : {radius, top_k, min_sources}) TORCH_CHECK(v >= 0 && v <= 0x7FFFFFFF, "sfm_hip: radius, top_k, min_sources must be in [0, 2^31)");
    const int64_t bytes = sfm_plane_sweep_workspace_bytes(d.V, d.H, d.W, d.R, d.S, d.D);
    TORCH_CHECK(bytes >= 0, "sfm_hip: sfm_plane_sweep refuses these sizes (need views >= 1, height and width >= 4, height * width < "
                            "2^31, refs <= 65535, 1 <= sources <= 8, 1 <= depths <= 4096)");
    Tensor ws = at::empty({bytes > 16 ? bytes : 16}, like(images, at::kByte));
    ok(sfm_plane_sweep(ptr<uint8_t>(images), d.V, d.H, d.W, ptr<double>(K), ptr<double>(poses), ptr<int32_t>(refs), d.R,
                       ptr<int32_t>(sources), d.S, ptr<double>(depths), d.D, (int)radius, (int)top_k, (int)min_sources, min_variance,
                       ptr<double>(depth), ptr<int32_t>(index), ptr<double>(cost), ptr<int32_t>(status),
                       with_volume ? ptr<double>(*volume) : nullptr, ws.data_ptr(), ws.numel(), current_stream()),
       "sfm_plane_sweep");
}

// the functional form -> (depth, index, cost, status, volume); volume is [refs, depths, height, width], or [0] when not asked for
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> plane_sweep_new(bool meta, const Tensor& images, const Tensor& K, const Tensor& poses,
                                                                   const Tensor& refs, const Tensor& sources, const Tensor& depths,
                                                                   int64_t radius, int64_t top_k, int64_t min_sources,
                                                                   double min_variance, bool return_volume) {
    TORCH_CHECK(images.dim() == 3 && refs.dim() == 1 && depths.dim() == 2, "sfm_hip: images must be [views, height, width], refs [refs], "
                                                                           "depths [refs, depths]");
    const SymInt R = refs.sym_size(0), H = images.sym_size(1), W = images.sym_size(2);
    Tensor depth = alloc(images, at::kDouble, {R, H, W}), cost = alloc(images, at::kDouble, {R, H, W});
    Tensor index = alloc(images, at::kInt, {R, H, W}), status = alloc(images, at::kInt, {R});
    Tensor volume = return_volume ? alloc(images, at::kDouble, {R, depths.sym_size(1), H, W}) : alloc(images, at::kDouble, {0});
    if (!meta)
        plane_sweep_out(images, K, poses, refs, sources, depths, radius, top_k, min_sources, min_variance, depth, index, cost, status,
                        return_volume ? std::optional<Tensor>(volume) : std::nullopt);
    return {depth, index, cost, status, volume};
}

void filter_depth_maps_out(const Tensor& depth, const Tensor& K, const Tensor& poses, const Tensor& refs, const Tensor& sources,
                           double max_pixel_error, double max_relative_depth_error, int64_t min_consistent, Tensor& count,
                           Tensor& filtered, Tensor& points, Tensor& status) {
    const OpDevice scope(depth);
    for (const Tensor* t : {&depth, &K, &poses}) need(*t, "depth / K / poses", at::kDouble);
    for (const Tensor* t : {&filtered, &points}) need(*t, "filtered / points", at::kDouble);
    for (const Tensor* t : {&refs, &sources}) need(*t, "refs / sources", at::kInt);
    for (const Tensor* t : {&count, &status}) need(*t, "count / status", at::kInt);
    const SweepDims d = sweep_dims(depth, K, poses, refs, sources);
    const int64_t pixels = d.R * d.H * d.W;
    TORCH_CHECK(count.numel() == pixels && filtered.numel() == pixels, "sfm_hip: count, filtered must be [refs, height, width]");
    TORCH_CHECK(points.numel() == 3 * pixels, "sfm_hip: points must be [refs, height, width, 3]");
    TORCH_CHECK(status.numel() == d.R, "sfm_hip: status must be int32 [refs]");
    TORCH_CHECK(min_consistent >= 0 && min_consistent <= 0x7FFFFFFF, "sfm_hip: min_consistent must be in [0, 2^31)");
    ok(sfm_filter_depth_maps(ptr<double>(depth), d.V, d.H, d.W, ptr<double>(K), ptr<double>(poses), ptr<int32_t>(refs), d.R,
                             ptr<int32_t>(sources), d.S, max_pixel_error, max_relative_depth_error, (int)min_consistent,
                             ptr<int32_t>(count), ptr<double>(filtered), ptr<double>(points), ptr<int32_t>(status), current_stream()),
       "sfm_filter_depth_maps");
}

// the functional form -> (count, filtered, points, status)
std::tuple<Tensor, Tensor, Tensor, Tensor> filter_depth_maps_new(bool meta, const Tensor& depth, const Tensor& K, const Tensor& poses,
                                                                 const Tensor& refs, const Tensor& sources, double max_pixel_error,
                                                                 double max_relative_depth_error, int64_t min_consistent) {
    TORCH_CHECK(depth.dim() == 3 && refs.dim() == 1, "sfm_hip: depth must be [views, height, width], refs [refs]");
    const SymInt R = refs.sym_size(0), H = depth.sym_size(1), W = depth.sym_size(2);
    Tensor count = alloc(depth, at::kInt, {R, H, W}), filtered = alloc(depth, at::kDouble, {R, H, W});
    Tensor points = alloc(depth, at::kDouble, {R, H, W, 3}), status = alloc(depth, at::kInt, {R});
    if (!meta)
        filter_depth_maps_out(depth, K, poses, refs, sources, max_pixel_error, max_relative_depth_error, min_consistent, count, filtered,
                              points, status);
    return {count, filtered, points, status};
}

// ---- semi-global smoothing of the plane-sweep cost volume (sfm_sgm.hip): volume [R, D, H, W] and depths [R, D] on the device; depth,
// cost [R, H, W], index int32 [R, H, W], aggregated [R, D, H, W] or none.  The workspace comes from the caching allocator ------------
void sgm_aggregate_out(const Tensor& volume, const Tensor& depths, double p1, double p2, double invalid_cost, int64_t paths, Tensor& depth,
                       Tensor& index, Tensor& cost, const std::optional<Tensor>& aggregated) {
    const OpDevice scope(volume);
    for (const Tensor* t : {&volume, &depths}) need(*t, "volume / depths", at::kDouble);
    for (const Tensor* t : {&depth, &cost}) need(*t, "depth / cost", at::kDouble);
    need(index, "index", at::kInt);
    TORCH_CHECK(volume.dim() == 4, "sfm_hip: volume must be [refs, depths, height, width]");
    const int64_t R = volume.size(0), D = volume.size(1), H = volume.size(2), W = volume.size(3);
    TORCH_CHECK(depths.dim() == 2 && depths.size(0) == R && depths.size(1) == D, "sfm_hip: depths must be [refs, depths]");
    const int64_t pixels = R * H * W;
    TORCH_CHECK(depth.numel() == pixels && cost.numel() == pixels && index.numel() == pixels,
                "sfm_hip: depth, index, cost must be [refs, height, width]");
    const bool keep = aggregated.has_value() && aggregated->defined();
    if (keep) {
        need(*aggregated, "aggregated", at::kDouble);
        TORCH_CHECK(aggregated->numel() == pixels * D, "sfm_hip: aggregated must be [refs, depths, height, width]");
    }
    TORCH_CHECK(paths >= 0 && paths <= 0x7FFFFFFF, "sfm_hip: paths must be 4 or 8");
    const int64_t bytes = sfm_sgm_workspace_bytes(R, D, H, W, keep ? 1 : 0);
    TORCH_CHECK(bytes >= 0, "sfm_hip: sfm_sgm_aggregate refuses these sizes (need refs <= 65535, 1 <= depths <= 256, height and width >= 1, "
                            "height * width < 2^31)");
    Tensor ws = at::empty({bytes > 16 ? bytes : 16}, like(volume, at::kByte));
    ok(sfm_sgm_aggregate(ptr<double>(volume), R, D, H, W, ptr<double>(depths), p1, p2, invalid_cost, (int)paths, ptr<double>(depth),
                         ptr<int32_t>(index), ptr<double>(cost), keep ? ptr<double>(*aggregated) : nullptr, ws.data_ptr(), ws.numel(),
                         current_stream()),
       "sfm_sgm_aggregate");
}

// the functional form -> (depth, index, cost, aggregated); aggregated is [refs, depths, height, width], or [0] when not asked for
std::tuple<Tensor, Tensor, Tensor, Tensor> sgm_aggregate_new(bool meta, const Tensor& volume, const Tensor& depths, double p1, double p2,
                                                             double invalid_cost, int64_t paths, bool return_aggregated) {
    TORCH_CHECK(volume.dim() == 4, "sfm_hip: volume must be [refs, depths, height, width]");
    const SymInt R = volume.sym_size(0), H = volume.sym_size(2), W = volume.sym_size(3);
    Tensor depth = alloc(volume, at::kDouble, {R, H, W}), cost = alloc(volume, at::kDouble, {R, H, W});
    Tensor index = alloc(volume, at::kInt, {R, H, W});
    Tensor aggregated = return_aggregated ? alloc(volume, at::kDouble, {R, volume.sym_size(1), H, W}) : alloc(volume, at::kDouble, {0});
    if (!meta)
        sgm_aggregate_out(volume, depths, p1, p2, invalid_cost, paths, depth, index, cost,
                          return_aggregated ? std::optional<Tensor>(aggregated) : std::nullopt);
    return {depth, index, cost, aggregated};
}

// ---- fusion of depth maps into a TSDF volume and its mesh (sfm_tsdf.hip): the state sum [nz, ny, nx], count int32, grey_sum int32 or
// none; depth [V, H, W], images uint8 [V, H, W] or none, K [9], poses [V, 12], views int32 [N]; vertices [T, 3, 3], grey [T, 3] or
// none, total int64 [1].  The mesh's workspace comes from the caching allocator --------------------------------------------------------
bool given(const std::optional<Tensor>& t) { return t.has_value() && t->defined(); }

void tsdf_state_check(const Tensor& sum, const Tensor& count, const std::optional<Tensor>& grey_sum) {
    need(sum, "sum", at::kDouble);
    need(count, "count", at::kInt);
    TORCH_CHECK(sum.dim() == 3 && count.sizes() == sum.sizes(), "sfm_hip: sum and count must be [nz, ny, nx]");
    if (given(grey_sum)) {
        need(*grey_sum, "grey_sum", at::kInt);
        TORCH_CHECK(grey_sum->sizes() == sum.sizes(), "sfm_hip: grey_sum must be [nz, ny, nx]");
    }
}

void tsdf_integrate_out(Tensor& sum, Tensor& count, const std::optional<Tensor>& grey_sum, const Tensor& depth,
                        const std::optional<Tensor>& images, const Tensor& K, const Tensor& poses, const Tensor& views, double ox, double oy,
                        double oz, double voxel_size, double truncation, Tensor& status) {
    const OpDevice scope(sum);
    tsdf_state_check(sum, count, grey_sum);
    for (const Tensor* t : {&depth, &K, &poses}) need(*t, "depth / K / poses", at::kDouble);
    need(views, "views", at::kInt);
    need(status, "status", at::kInt);
    TORCH_CHECK(depth.dim() == 3, "sfm_hip: depth must be [views, height, width]");
    TORCH_CHECK(K.numel() == 9, "sfm_hip: K must hold 9 doubles");
    TORCH_CHECK(poses.dim() == 2 && poses.size(0) == depth.size(0) && poses.size(1) == 12, "sfm_hip: poses must be [views, 12]");
    TORCH_CHECK(views.dim() == 1 && status.numel() == views.numel(), "sfm_hip: views and status must be int32 [n]");
    TORCH_CHECK(given(images) == given(grey_sum), "sfm_hip: images must be given exactly when grey_sum is");
    if (given(images)) {
        need(*images, "images", at::kByte);
        TORCH_CHECK(images->sizes() == depth.sizes(), "sfm_hip: images must be [views, height, width] like depth");
    }
    TORCH_CHECK(sum.numel() > 0 && depth.numel() > 0, "sfm_hip: the volume and the depth maps must not be empty");
    ok(sfm_tsdf_integrate(ptr<double>(sum), ptr<int32_t>(count), ptr<int32_t>(grey_sum), sum.size(2), sum.size(1), sum.size(0), ox, oy, oz,
                          voxel_size, truncation, ptr<double>(depth), ptr<uint8_t>(images), depth.size(0), depth.size(1), depth.size(2),
                          ptr<double>(K), ptr<double>(poses), ptr<int32_t>(views), views.numel(), ptr<int32_t>(status), current_stream()),
       "sfm_tsdf_integrate");
}

// the functional form -> (sum, count, grey_sum, status): new tensors; grey_sum is [0] without one
std::tuple<Tensor, Tensor, Tensor, Tensor> tsdf_integrate_new(bool meta, const Tensor& sum, const Tensor& count,
                                                              const std::optional<Tensor>& grey_sum, const Tensor& depth,
                                                              const std::optional<Tensor>& images, const Tensor& K, const Tensor& poses,
                                                              const Tensor& views, double ox, double oy, double oz, double voxel_size,
                                                              double truncation) {
    TORCH_CHECK(views.dim() == 1, "sfm_hip: views must be int32 [n]");
    auto copy = [meta](const Tensor& t) { return meta ? at::empty_like(t) : t.clone(); };   // the state the call goes on from
    Tensor new_sum = copy(sum), new_count = copy(count);
    Tensor new_grey = given(grey_sum) ? copy(*grey_sum) : alloc(sum, at::kInt, {0});
    Tensor status = alloc(sum, at::kInt, {views.sym_size(0)});
    if (!meta)
        tsdf_integrate_out(new_sum, new_count, given(grey_sum) ? std::optional<Tensor>(new_grey) : std::nullopt, depth, images, K, poses,
                           views, ox, oy, oz, voxel_size, truncation, status);
    return {new_sum, new_count, new_grey, status};
}

void tsdf_extract_mesh_out(const Tensor& sum, const Tensor& count, const std::optional<Tensor>& grey_sum, double ox, double oy, double oz,
                           double voxel_size, int64_t min_count, Tensor& vertices, const std::optional<Tensor>& grey, Tensor& total) {
    const OpDevice scope(sum);
    tsdf_state_check(sum, count, grey_sum);
    need(vertices, "vertices", at::kDouble);
    need(total, "total", at::kLong);
    TORCH_CHECK(vertices.dim() == 3 && vertices.size(1) == 3 && vertices.size(2) == 3, "sfm_hip: vertices must be [max_triangles, 3, 3]");
    TORCH_CHECK(total.numel() == 1, "sfm_hip: total must be int64 [1]");
    TORCH_CHECK(given(grey) == given(grey_sum), "sfm_hip: grey must be given exactly when grey_sum is");
    const int64_t T = vertices.size(0);
    if (given(grey)) {
        need(*grey, "grey", at::kDouble);
        TORCH_CHECK(grey->dim() == 2 && grey->size(0) == T && grey->size(1) == 3, "sfm_hip: grey must be [max_triangles, 3]");
    }
    TORCH_CHECK(min_count >= 1 && min_count <= 0x7FFFFFFF, "sfm_hip: min_count must be in [1, 2^31)");
    const int64_t bytes = sfm_tsdf_mesh_workspace_bytes(sum.size(2), sum.size(1), sum.size(0));
    TORCH_CHECK(bytes >= 0, "sfm_hip: sfm_tsdf_extract_mesh refuses these sizes (need nx, ny, nz >= 2, nx ny nz < 2^31 and "
                            "12 (nx-1)(ny-1)(nz-1) < 2^31)");
    Tensor ws = at::empty({bytes > 16 ? bytes : 16}, like(sum, at::kByte));
    // with no row to write the entry point takes no grey either: a [0, 3] tensor has no address
    ok(sfm_tsdf_extract_mesh(ptr<double>(sum), ptr<int32_t>(count), ptr<int32_t>(grey_sum), sum.size(2), sum.size(1), sum.size(0), ox, oy,
                             oz, voxel_size, (int)min_count, T, ptr<double>(vertices), ptr<double>(grey), ptr<int64_t>(total),
                             ws.data_ptr(), ws.numel(), current_stream()),
       "sfm_tsdf_extract_mesh");
}

// the functional form -> (vertices, grey, total); grey is [0] without a grey_sum
std::tuple<Tensor, Tensor, Tensor> tsdf_extract_mesh_new(bool meta, const Tensor& sum, const Tensor& count,
                                                         const std::optional<Tensor>& grey_sum, double ox, double oy, double oz,
                                                         double voxel_size, int64_t min_count, int64_t max_triangles) {
    if (!meta) TORCH_CHECK(max_triangles >= 0, "sfm_hip: max_triangles must be >= 0");
    Tensor vertices = alloc(sum, at::kDouble, {max_triangles, 3, 3}), total = alloc(sum, at::kLong, {1});
    Tensor grey = given(grey_sum) ? alloc(sum, at::kDouble, {max_triangles, 3}) : alloc(sum, at::kDouble, {0});
    if (!meta)
        tsdf_extract_mesh_out(sum, count, grey_sum, ox, oy, oz, voxel_size, min_count, vertices,
                              given(grey_sum) ? std::optional<Tensor>(grey) : std::nullopt, total);
    return {vertices, grey, total};
}

// bundle adjustment, dense (sfm_bundle.hip) and with the iterative Schur solver (sfm_bundle_pcg.hip): poses [C, 12], points
// [P, 3], camera / point indices int32 [M], pixels [M, 2]; fixed: the indices of the fixed cameras; the iterative solver takes
// max_cg_iterations and cg_tolerance as well; info int64 [4] viewing the sfm_bundle_info record, int64 [5] viewing
// sfm_bundle_pcg_info.  The workspace comes from the caching allocator, stream-ordered like everything else; the dense solver
// does not synchronise the host, the iterative one synchronises the stream (the host reads the LM and CG stop flags).
// The `_robust` ops add a loss (SFM_BUNDLE_LOSS_*, csrc/sfm_loss.h) and its scale in pixels: new ops, so that no existing
// schema changes.  Four op families, each functional, in-place and Meta, over one body.
void loss_check(int64_t loss, double loss_scale) {
    TORCH_CHECK(loss >= SFM_BUNDLE_LOSS_SQUARED && loss <= SFM_BUNDLE_LOSS_CAUCHY, "sfm_hip: loss must be 0 (squared), 1 (huber) or 2 (cauchy)");
    TORCH_CHECK(sfmloss::scale_ok(loss_scale), "sfm_hip: loss_scale must be positive with a normal finite square");
}

sfm_bundle_options bundle_options(int64_t loss, double loss_scale) {
    loss_check(loss, loss_scale);
    return sfm_bundle_options{(int32_t)loss, 0, loss_scale};
}

// Which adjuster a call runs: the dense one (max_cg_iterations and cg_tolerance unread) or the iterative one; options: null
// for the ops without a loss
struct BundleSolver {
    bool pcg;
    int64_t max_cg_iterations;
    double cg_tolerance;
    const sfm_bundle_options* options;
    int64_t info_words() const { return (pcg ? sizeof(sfm_bundle_pcg_info) : sizeof(sfm_bundle_info)) / 8; }
};

void bundle_check(const BundleSolver& s, const Tensor& poses, const Tensor& points, const Tensor& cam, const Tensor& pt,
                  const Tensor& pixels, at::ArrayRef<double> K, at::ArrayRef<int64_t> fixed, int64_t max_steps) {
    check_K(K);
    TORCH_CHECK(poses.dim() == 2 && poses.size(1) == 12, "sfm_hip: poses must be [C, 12]");
    TORCH_CHECK(points.dim() == 2 && points.size(1) == 3, "sfm_hip: points must be [P, 3]");
    TORCH_CHECK(cam.dim() == 1 && pt.dim() == 1 && cam.size(0) == pt.size(0), "sfm_hip: camera and point indices must be [M]");
    TORCH_CHECK(pixels.dim() == 2 && pixels.size(1) == 2 && pixels.size(0) == cam.size(0), "sfm_hip: pixels must be [M, 2]");
    TORCH_CHECK(max_steps >= 0 && max_steps <= 0x7FFFFFFF, "sfm_hip: max_steps must be in [0, 2^31)");
    for (int64_t c : fixed) TORCH_CHECK(c >= 0 && c < poses.size(0), "sfm_hip: fixed camera ", c, " out of range");
    if (!s.pcg) return;
    TORCH_CHECK(s.max_cg_iterations >= 1 && s.max_cg_iterations <= 0x7FFFFFFF, "sfm_hip: max_cg_iterations must be in [1, 2^31)");
    TORCH_CHECK(s.cg_tolerance > 0.0 && s.cg_tolerance < 1.0, "sfm_hip: cg_tolerance must be in (0, 1)");
}

// The in-place form: poses_in / points_in are the start, poses / points the result (the same tensors for the `_` ops).  The
// plain entry points forward to the _ex ones with null options, so the _ex ones serve every call.
void bundle_run(const BundleSolver& s, Tensor& poses, Tensor& points, const Tensor& cam, const Tensor& pt, const Tensor& pixels,
                at::ArrayRef<double> K, at::ArrayRef<int64_t> fixed, int64_t max_steps, Tensor& info, const Tensor& poses_in,
                const Tensor& points_in) {
    const OpDevice scope(poses);
    need(poses, "poses", at::kDouble);
    need(points, "points", at::kDouble);
    need(poses_in, "poses", at::kDouble);
    need(points_in, "points", at::kDouble);
    need(cam, "camera_indices", at::kInt);
    need(pt, "point_indices", at::kInt);
    need(pixels, "pixels", at::kDouble);
    need(info, "info", at::kLong);
    bundle_check(s, poses_in, points_in, cam, pt, pixels, K, fixed, max_steps);
    TORCH_CHECK(poses.sizes() == poses_in.sizes() && points.sizes() == points_in.sizes(), "sfm_hip: output shapes differ");
    TORCH_CHECK(info.numel() == s.info_words(), "sfm_hip: info must be int64 [", s.info_words(), "]");
    const int64_t C = poses.size(0), P = points.size(0), M = cam.size(0);
    std::vector<uint8_t> mask((size_t)C, 0);
    for (int64_t c : fixed) mask[(size_t)c] = 1;
    const int64_t bytes = s.pcg ? sfm_bundle_pcg_workspace_bytes_ex(C, P, M, s.options) : sfm_bundle_workspace_bytes(C, P, M);
    TORCH_CHECK(bytes >= 0, "sfm_hip: ", s.pcg ? "bundle_adjust_pcg: " : "bundle_adjust: ", C, " cameras, ", P, " points, ", M,
                " observations exceed the limits ", s.pcg ? "(C >= 1; C, P and M < 2^31)" : "(C <= 64, P and M < 2^31)");
    Tensor ws = at::empty({bytes}, like(poses, at::kByte));
    void* const record = ptr<int64_t>(info);
    if (s.pcg)
        ok(sfm_bundle_adjust_pcg_ex(K.data(), C, P, M, mask.data(), ptr<double>(poses_in), ptr<double>(points_in),
                                    ptr<int32_t>(cam), ptr<int32_t>(pt), ptr<double>(pixels), (int)max_steps,
                                    (int)s.max_cg_iterations, s.cg_tolerance, ptr<double>(poses), ptr<double>(points),
                                    static_cast<sfm_bundle_pcg_info*>(record), ws.data_ptr(), bytes, current_stream(), s.options),
           s.options ? "sfm_bundle_adjust_pcg_ex" : "sfm_bundle_adjust_pcg");
    else
        ok(sfm_bundle_adjust_ex(K.data(), C, P, M, mask.data(), ptr<double>(poses_in), ptr<double>(points_in),
                                ptr<int32_t>(cam), ptr<int32_t>(pt), ptr<double>(pixels), (int)max_steps, ptr<double>(poses),
                                ptr<double>(points), static_cast<sfm_bundle_info*>(record), ws.data_ptr(), bytes,
                                current_stream(), s.options),
           s.options ? "sfm_bundle_adjust_ex" : "sfm_bundle_adjust");
}

using BundleResult = std::tuple<Tensor, Tensor, Tensor>;

// The functional form; `meta`: the shapes of the results only
BundleResult bundle_new(const BundleSolver& s, bool meta, const Tensor& poses, const Tensor& points, const Tensor& cam,
                        const Tensor& pt, const Tensor& pixels, at::ArrayRef<double> K, at::ArrayRef<int64_t> fixed,
                        int64_t max_steps) {
    bundle_check(s, poses, points, cam, pt, pixels, K, fixed, max_steps);
    Tensor poses_out = at::empty_like(poses);
    Tensor points_out = at::empty_like(points);
    Tensor info = at::empty_symint({c10::SymInt(s.info_words())}, like(poses, at::kLong));
    if (!meta) bundle_run(s, poses_out, points_out, cam, pt, pixels, K, fixed, max_steps, info, poses, points);
    return {poses_out, points_out, info};
}

// The four families: each names its solver and forwards, in place and functional
void bundle_adjust_out(Tensor& poses, Tensor& points, const Tensor& cam, const Tensor& pt, const Tensor& pixels,
                       at::ArrayRef<double> K, at::ArrayRef<int64_t> fixed, int64_t max_steps, Tensor& info) {
    bundle_run({false, 0, 0.0, nullptr}, poses, points, cam, pt, pixels, K, fixed, max_steps, info, poses, points);
}

BundleResult bundle_adjust_new(bool meta, const Tensor& poses, const Tensor& points, const Tensor& cam, const Tensor& pt,
                               const Tensor& pixels, at::ArrayRef<double> K, at::ArrayRef<int64_t> fixed, int64_t max_steps) {
    return bundle_new({false, 0, 0.0, nullptr}, meta, poses, points, cam, pt, pixels, K, fixed, max_steps);
}

void bundle_adjust_pcg_out(Tensor& poses, Tensor& points, const Tensor& cam, const Tensor& pt, const Tensor& pixels,
                           at::ArrayRef<double> K, at::ArrayRef<int64_t> fixed, int64_t max_steps, int64_t max_cg_iterations,
                           double cg_tolerance, Tensor& info) {
    bundle_run({true, max_cg_iterations, cg_tolerance, nullptr}, poses, points, cam, pt, pixels, K, fixed, max_steps, info, poses,
               points);
}

BundleResult bundle_adjust_pcg_new(bool meta, const Tensor& poses, const Tensor& points, const Tensor& cam, const Tensor& pt,
                                   const Tensor& pixels, at::ArrayRef<double> K, at::ArrayRef<int64_t> fixed, int64_t max_steps,
                                   int64_t max_cg_iterations, double cg_tolerance) {
    return bundle_new({true, max_cg_iterations, cg_tolerance, nullptr}, meta, poses, points, cam, pt, pixels, K, fixed, max_steps);
}

void bundle_adjust_robust_out(Tensor& poses, Tensor& points, const Tensor& cam, const Tensor& pt, const Tensor& pixels,
                              at::ArrayRef<double> K, at::ArrayRef<int64_t> fixed, int64_t max_steps, int64_t loss,
                              double loss_scale, Tensor& info) {
    const sfm_bundle_options options = bundle_options(loss, loss_scale);
    bundle_run({false, 0, 0.0, &options}, poses, points, cam, pt, pixels, K, fixed, max_steps, info, poses, points);
}

BundleResult bundle_adjust_robust_new(bool meta, const Tensor& poses, const Tensor& points, const Tensor& cam, const Tensor& pt,
                                      const Tensor& pixels, at::ArrayRef<double> K, at::ArrayRef<int64_t> fixed, int64_t max_steps,
                                      int64_t loss, double loss_scale) {
    const sfm_bundle_options options = bundle_options(loss, loss_scale);
    return bundle_new({false, 0, 0.0, &options}, meta, poses, points, cam, pt, pixels, K, fixed, max_steps);
}

void bundle_adjust_pcg_robust_out(Tensor& poses, Tensor& points, const Tensor& cam, const Tensor& pt, const Tensor& pixels,
                                  at::ArrayRef<double> K, at::ArrayRef<int64_t> fixed, int64_t max_steps, int64_t max_cg_iterations,
                                  double cg_tolerance, int64_t loss, double loss_scale, Tensor& info) {
    const sfm_bundle_options options = bundle_options(loss, loss_scale);
    bundle_run({true, max_cg_iterations, cg_tolerance, &options}, poses, points, cam, pt, pixels, K, fixed, max_steps, info, poses,
               points);
}

BundleResult bundle_adjust_pcg_robust_new(bool meta, const Tensor& poses, const Tensor& points, const Tensor& cam, const Tensor& pt,
                                          const Tensor& pixels, at::ArrayRef<double> K, at::ArrayRef<int64_t> fixed,
                                          int64_t max_steps, int64_t max_cg_iterations, double cg_tolerance, int64_t loss,
                                          double loss_scale) {
    const sfm_bundle_options options = bundle_options(loss, loss_scale);
    return bundle_new({true, max_cg_iterations, cg_tolerance, &options}, meta, poses, points, cam, pt, pixels, K, fixed, max_steps);
}

// The calibrating dense adjuster (sfm_bundle_adjust_calibrated): the arguments of bundle_adjust_robust plus the
// SFM_BUNDLE_REFINE_* bits; a fourth result, the refined camera matrix [3, 3].  Enqueue-only like bundle_adjust.
using BundleCalibratedResult = std::tuple<Tensor, Tensor, Tensor, Tensor>;

sfm_bundle_calibration_options calibration_options(int64_t loss, double loss_scale, int64_t refine) {
    TORCH_CHECK(refine >= 1 && refine <= (SFM_BUNDLE_REFINE_FOCAL | SFM_BUNDLE_REFINE_PRINCIPAL_POINT),
                "sfm_hip: refine must be 1 (focal), 2 (principal point) or 3 (both)");
    return sfm_bundle_calibration_options{bundle_options(loss, loss_scale), (int32_t)refine, 0};
}

void bundle_calibrated_run(Tensor& poses, Tensor& points, const Tensor& cam, const Tensor& pt, const Tensor& pixels,
                           at::ArrayRef<double> K, at::ArrayRef<int64_t> fixed, int64_t max_steps, int64_t loss, double loss_scale,
                           int64_t refine, Tensor& info, Tensor& K_out, const Tensor& poses_in, const Tensor& points_in) {
    const sfm_bundle_calibration_options options = calibration_options(loss, loss_scale, refine);
    const BundleSolver s{false, 0, 0.0, &options.loss};
    const OpDevice scope(poses);
    need(poses, "poses", at::kDouble);
    need(points, "points", at::kDouble);
    need(poses_in, "poses", at::kDouble);
    need(points_in, "points", at::kDouble);
    need(cam, "camera_indices", at::kInt);
    need(pt, "point_indices", at::kInt);
    need(pixels, "pixels", at::kDouble);
    need(info, "info", at::kLong);
    need(K_out, "K_out", at::kDouble);
    bundle_check(s, poses_in, points_in, cam, pt, pixels, K, fixed, max_steps);
    TORCH_CHECK(poses.sizes() == poses_in.sizes() && points.sizes() == points_in.sizes(), "sfm_hip: output shapes differ");
    TORCH_CHECK(info.numel() == s.info_words(), "sfm_hip: info must be int64 [", s.info_words(), "]");
    TORCH_CHECK(K_out.numel() == 9, "sfm_hip: K_out must be [3, 3]");
    const int64_t C = poses.size(0), P = points.size(0), M = cam.size(0);
    std::vector<uint8_t> mask((size_t)C, 0);
    for (int64_t c : fixed) mask[(size_t)c] = 1;
    const int64_t bytes = sfm_bundle_calibrated_workspace_bytes(C, P, M);
    TORCH_CHECK(bytes >= 0, "sfm_hip: bundle_adjust_calibrated: ", C, " cameras, ", P, " points, ", M,
                " observations exceed the limits (C <= 64, P and M < 2^31)");
    Tensor ws = at::empty({bytes}, like(poses, at::kByte));
    ok(sfm_bundle_adjust_calibrated(K.data(), C, P, M, mask.data(), ptr<double>(poses_in), ptr<double>(points_in),
                                    ptr<int32_t>(cam), ptr<int32_t>(pt), ptr<double>(pixels), (int)max_steps, ptr<double>(poses),
                                    ptr<double>(points), static_cast<sfm_bundle_info*>(static_cast<void*>(ptr<int64_t>(info))),
                                    ptr<double>(K_out), ws.data_ptr(), bytes, current_stream(), &options),
       "sfm_bundle_adjust_calibrated");
}

BundleCalibratedResult bundle_calibrated_new(bool meta, const Tensor& poses, const Tensor& points, const Tensor& cam,
                                             const Tensor& pt, const Tensor& pixels, at::ArrayRef<double> K,
                                             at::ArrayRef<int64_t> fixed, int64_t max_steps, int64_t loss, double loss_scale,
                                             int64_t refine) {
    const sfm_bundle_calibration_options options = calibration_options(loss, loss_scale, refine);
    const BundleSolver s{false, 0, 0.0, &options.loss};
    bundle_check(s, poses, points, cam, pt, pixels, K, fixed, max_steps);
    Tensor poses_out = at::empty_like(poses);
    Tensor points_out = at::empty_like(points);
    Tensor info = at::empty_symint({c10::SymInt(s.info_words())}, like(poses, at::kLong));
    Tensor K_out = at::empty_symint({c10::SymInt(3), c10::SymInt(3)}, like(poses, at::kDouble));
    if (!meta)
        bundle_calibrated_run(poses_out, points_out, cam, pt, pixels, K, fixed, max_steps, loss, loss_scale, refine, info, K_out,
                              poses, points);
    return {poses_out, points_out, info, K_out};
}

void bundle_adjust_calibrated_out(Tensor& poses, Tensor& points, const Tensor& cam, const Tensor& pt, const Tensor& pixels,
                                  at::ArrayRef<double> K, at::ArrayRef<int64_t> fixed, int64_t max_steps, int64_t loss,
                                  double loss_scale, int64_t refine, Tensor& info, Tensor& K_out) {
    bundle_calibrated_run(poses, points, cam, pt, pixels, K, fixed, max_steps, loss, loss_scale, refine, info, K_out, poses,
                          points);
}

// triangulation of multi-view tracks (sfm_tracks.hip): poses [C, 12], camera / point indices int32 [M], pixels [M, 2],
// `points` the number of points P -> points [P, 3], status uint8 [P], obs_error [M], angle [P] (radians), info int64 [4]
// viewing the sfm_tracks_info record.  The workspace comes from the caching allocator (stream-ordered, no host sync).
constexpr int64_t kTracksInfoWords = sizeof(sfm_tracks_info) / 8;

void tracks_check(const Tensor& poses, const Tensor& cam, const Tensor& pt, const Tensor& pixels, int64_t points,
                  at::ArrayRef<double> K, int64_t min_views, double min_angle, double max_error, int64_t refine_steps) {
    check_K(K);
    TORCH_CHECK(poses.dim() == 2 && poses.size(1) == 12, "sfm_hip: poses must be [C, 12]");
    TORCH_CHECK(cam.dim() == 1 && pt.dim() == 1 && cam.size(0) == pt.size(0), "sfm_hip: camera and point indices must be [M]");
    TORCH_CHECK(pixels.dim() == 2 && pixels.size(1) == 2 && pixels.size(0) == cam.size(0), "sfm_hip: pixels must be [M, 2]");
    TORCH_CHECK(points >= 0 && points < 0x7FFFFFFF, "sfm_hip: points must be in [0, 2^31 - 1)");
    TORCH_CHECK(min_views >= 2 && min_views <= 0x7FFFFFFF, "sfm_hip: min_views must be at least 2");
    TORCH_CHECK(min_angle >= 0.0 && std::isfinite(min_angle), "sfm_hip: min_angle must be finite and >= 0");
    TORCH_CHECK(max_error >= 0.0, "sfm_hip: max_error must be >= 0");
    TORCH_CHECK(refine_steps >= 0 && refine_steps <= 0x7FFFFFFF, "sfm_hip: refine_steps must be in [0, 2^31)");
}

void triangulate_tracks_out(const Tensor& poses, const Tensor& cam, const Tensor& pt, const Tensor& pixels, int64_t points,
                            at::ArrayRef<double> K, int64_t min_views, double min_angle, double max_error,
                            int64_t refine_steps, Tensor& points_out, Tensor& status, Tensor& obs_error, Tensor& angle,
                            Tensor& info) {
    const OpDevice scope(poses);
    need(poses, "poses", at::kDouble);
    need(cam, "camera_indices", at::kInt);
    need(pt, "point_indices", at::kInt);
    need(pixels, "pixels", at::kDouble);
    need(points_out, "points", at::kDouble);
    need(status, "status", at::kByte);
    need(obs_error, "obs_error", at::kDouble);
    need(angle, "angle", at::kDouble);
    need(info, "info", at::kLong);
    tracks_check(poses, cam, pt, pixels, points, K, min_views, min_angle, max_error, refine_steps);
    const int64_t C = poses.size(0), P = points, M = cam.size(0);
    TORCH_CHECK(points_out.dim() == 2 && points_out.size(0) == P && points_out.size(1) == 3, "sfm_hip: points must be [P, 3]");
    TORCH_CHECK(status.numel() == P && angle.numel() == P, "sfm_hip: status and angle must be [P]");
    TORCH_CHECK(obs_error.numel() == M, "sfm_hip: obs_error must be [M]");
    TORCH_CHECK(info.numel() == kTracksInfoWords, "sfm_hip: info must be int64 [4]");
    const int64_t bytes = sfm_tracks_workspace_bytes(P, M);
    TORCH_CHECK(bytes >= 0, "sfm_hip: triangulate_tracks: ", P, " points, ", M, " observations exceed the limits");
    Tensor ws = at::empty({bytes}, like(poses, at::kByte));
    ok(sfm_triangulate_tracks(K.data(), C, P, M, ptr<double>(poses), ptr<int32_t>(cam), ptr<int32_t>(pt), ptr<double>(pixels),
                              (int)min_views, min_angle, max_error, (int)refine_steps, ptr<double>(points_out),
                              ptr<uint8_t>(status), ptr<double>(obs_error), ptr<double>(angle),
                              reinterpret_cast<sfm_tracks_info*>(ptr<int64_t>(info)), ws.data_ptr(), bytes, current_stream()),
       "sfm_triangulate_tracks");
}

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> triangulate_tracks_new(bool meta, const Tensor& poses, const Tensor& cam,
                                                                          const Tensor& pt, const Tensor& pixels, int64_t points,
                                                                          at::ArrayRef<double> K, int64_t min_views, double min_angle,
                                                                          double max_error, int64_t refine_steps) {
    tracks_check(poses, cam, pt, pixels, points, K, min_views, min_angle, max_error, refine_steps);
    Tensor points_out = alloc(poses, at::kDouble, {points, 3});
    Tensor status = alloc(poses, at::kByte, {points});
    Tensor obs_error = alloc(poses, at::kDouble, {cam.sym_size(0)});
    Tensor angle = alloc(poses, at::kDouble, {points});
    Tensor info = alloc(poses, at::kLong, {kTracksInfoWords});
    if (!meta)
        triangulate_tracks_out(poses, cam, pt, pixels, points, K, min_views, min_angle, max_error, refine_steps, points_out, status,
                               obs_error, angle, info);
    return {points_out, status, obs_error, angle, info};
}

// tracks from pairwise matches (sfm_track_build.hip): image_offset int32 [I + 1], pair_images int32 [Q, 2], match_offset
// int32 [Q + 1], match_index int32 [E, 2] (local indices), `features` = F -> component, track int32 [F], status uint8 [F],
// camera_index, point_index, feature_index int32 [F] (the first info.observations valid, the rest -1), info int64 [6]
// viewing the sfm_build_tracks_info record.  The workspace comes from the caching allocator (stream-ordered, no host sync).
constexpr int64_t kBuildInfoWords = sizeof(sfm_build_tracks_info) / 8;

void build_check(const Tensor& image_offset, const Tensor& pair_images, const Tensor& match_offset, const Tensor& match_index,
                 int64_t features) {
    TORCH_CHECK(image_offset.dim() == 1 && image_offset.size(0) >= 1, "sfm_hip: image_offset must be [I + 1]");
    TORCH_CHECK(pair_images.dim() == 2 && pair_images.size(1) == 2, "sfm_hip: pair_images must be [Q, 2]");
    TORCH_CHECK(match_offset.dim() == 1 && match_offset.size(0) == pair_images.size(0) + 1, "sfm_hip: match_offset must be [Q + 1]");
    TORCH_CHECK(match_index.dim() == 2 && match_index.size(1) == 2, "sfm_hip: match_index must be [E, 2]");
    TORCH_CHECK(features >= 0 && features < 0x7FFFFFFF, "sfm_hip: features must be in [0, 2^31 - 1)");
}

void build_tracks_out(const Tensor& image_offset, const Tensor& pair_images, const Tensor& match_offset, const Tensor& match_index,
                      int64_t features, Tensor& component, Tensor& track, Tensor& status, Tensor& camera_index,
                      Tensor& point_index, Tensor& feature_index, Tensor& info) {
    const OpDevice scope(image_offset);
    need(image_offset, "image_offset", at::kInt);
    need(pair_images, "pair_images", at::kInt);
    need(match_offset, "match_offset", at::kInt);
    need(match_index, "match_index", at::kInt);
    need(component, "component", at::kInt);
    need(track, "track", at::kInt);
    need(status, "status", at::kByte);
    need(camera_index, "camera_index", at::kInt);
    need(point_index, "point_index", at::kInt);
    need(feature_index, "feature_index", at::kInt);
    need(info, "info", at::kLong);
    build_check(image_offset, pair_images, match_offset, match_index, features);
    const int64_t I = image_offset.size(0) - 1, F = features, Q = pair_images.size(0), E = match_index.size(0);
    for (const Tensor* t : {&component, &track, &camera_index, &point_index, &feature_index, &status})
        TORCH_CHECK(t->dim() == 1 && t->size(0) == F, "sfm_hip: build_tracks outputs must be [features]");
    TORCH_CHECK(info.numel() == kBuildInfoWords, "sfm_hip: info must be int64 [6]");
    const int64_t bytes = sfm_build_tracks_workspace_bytes(I, F, E);
    TORCH_CHECK(bytes >= 0, "sfm_hip: build_tracks: ", I, " images, ", F, " features, ", E, " matches exceed the limits");
    Tensor ws = at::empty({bytes}, like(image_offset, at::kByte));
    ok(sfm_build_tracks(I, F, Q, E, ptr<int32_t>(image_offset), ptr<int32_t>(pair_images), ptr<int32_t>(match_offset),
                        ptr<int32_t>(match_index), ptr<int32_t>(component), ptr<int32_t>(track), ptr<uint8_t>(status),
                        ptr<int32_t>(camera_index), ptr<int32_t>(point_index), ptr<int32_t>(feature_index),
                        reinterpret_cast<sfm_build_tracks_info*>(ptr<int64_t>(info)), ws.data_ptr(), bytes, current_stream()),
       "sfm_build_tracks");
}

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> build_tracks_new(bool meta, const Tensor& image_offset,
                                                                                    const Tensor& pair_images,
                                                                                    const Tensor& match_offset,
                                                                                    const Tensor& match_index, int64_t features) {
    build_check(image_offset, pair_images, match_offset, match_index, features);
    auto i32 = [&] { return alloc(image_offset, at::kInt, {features}); };
    Tensor component = i32(), track = i32(), camera_index = i32(), point_index = i32(), feature_index = i32();
    Tensor status = alloc(image_offset, at::kByte, {features});
    Tensor info = alloc(image_offset, at::kLong, {kBuildInfoWords});
    if (!meta)
        build_tracks_out(image_offset, pair_images, match_offset, match_index, features, component, track, status, camera_index,
                         point_index, feature_index, info);
    return {component, track, status, camera_index, point_index, feature_index, info};
}

// What the solvers over a view graph check alike; `op` names the solver in the refusal of the sizes
void graph_solver_check(const char* op, const Tensor& pairs, const Tensor& weights, int64_t cameras, int64_t root, int64_t loss,
                        double loss_scale, int64_t max_steps, int64_t max_cg_iterations, double cg_tolerance,
                        double step_tolerance) {
    TORCH_CHECK(pairs.dim() == 2 && pairs.size(1) == 2, "sfm_hip: pairs must be [Q, 2]");
    TORCH_CHECK(weights.dim() == 1 && weights.size(0) == pairs.size(0), "sfm_hip: weights must be [Q]");
    TORCH_CHECK(cameras >= 1 && cameras <= 0x7FFFFFFF && pairs.size(0) < ((int64_t)1 << 30), "sfm_hip: ", op,
                ": cameras must be in [1, 2^31) and edges below 2^30");
    TORCH_CHECK(root >= 0 && root < cameras, "sfm_hip: root must be a camera index");
    loss_check(loss, loss_scale);
    TORCH_CHECK(max_steps >= 0 && max_steps <= 0x7FFFFFFF, "sfm_hip: max_steps must be in [0, 2^31)");
    TORCH_CHECK(max_cg_iterations >= 1 && max_cg_iterations <= 0x7FFFFFFF, "sfm_hip: max_cg_iterations must be in [1, 2^31)");
    TORCH_CHECK(cg_tolerance > 0.0 && cg_tolerance < 1.0, "sfm_hip: cg_tolerance must be in (0, 1)");
    TORCH_CHECK(step_tolerance > 0.0 && std::isfinite(step_tolerance), "sfm_hip: step_tolerance must be finite and positive");
}

// A table of rotations: [rows, 9] or [rows, 3, 3]; `rows_text` is how the message writes the row count
void rotation_table_check(const Tensor& t, int64_t rows, const char* name, const char* rows_text) {
    TORCH_CHECK((t.dim() == 2 && t.size(0) == rows && t.size(1) == 9) ||
                    (t.dim() == 3 && t.size(0) == rows && t.size(1) == 3 && t.size(2) == 3),
                "sfm_hip: ", name, " must be [", rows_text, ", 9] or [", rows_text, ", 3, 3]");
}

// rotation averaging over a view graph (sfm_rotation_averaging.hip): pairs int32 [Q, 2], relative f64 [Q, 9] or [Q, 3, 3],
// weights f64 [Q], `cameras` = C, the root, initial f64 [C, 9] or [C, 3, 3] (given: the start; None: the spanning tree), the
// loss (SFM_BUNDLE_LOSS_*) with its scale in radians and the limits -> rotations f64 [C, 3, 3], registered uint8 [C],
// level int32 [C] (-1: unregistered), residual f64 [Q] (radians), info int64 [5] viewing the sfm_rotavg_info record.  The call
// synchronises the stream (the host reads the stop flags).
constexpr int64_t kRotavgInfoWords = sizeof(sfm_rotavg_info) / 8;

void rotavg_check(const Tensor& pairs, const Tensor& relative, const Tensor& weights, int64_t cameras, int64_t root,
                  const std::optional<Tensor>& initial, int64_t loss, double loss_scale, int64_t max_steps,
                  int64_t max_cg_iterations, double cg_tolerance, double step_tolerance) {
    graph_solver_check("average_rotations", pairs, weights, cameras, root, loss, loss_scale, max_steps, max_cg_iterations,
                       cg_tolerance, step_tolerance);
    rotation_table_check(relative, pairs.size(0), "relative", "Q");
    if (initial.has_value() && initial->defined()) rotation_table_check(*initial, cameras, "initial", "cameras");
}

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> average_rotations_new(bool meta, const Tensor& pairs, const Tensor& relative,
                                                                         const Tensor& weights, int64_t cameras, int64_t root,
                                                                         const std::optional<Tensor>& initial, int64_t loss,
                                                                         double loss_scale, int64_t max_steps, int64_t max_cg_iterations,
                                                                         double cg_tolerance, double step_tolerance) {
    const OpDevice scope(pairs, meta);
    const bool given = initial.has_value() && initial->defined();
    if (!meta) {
        need(pairs, "pairs", at::kInt);
        need(relative, "relative", at::kDouble);
        need(weights, "weights", at::kDouble);
        if (given) need(*initial, "initial", at::kDouble);
    }
    rotavg_check(pairs, relative, weights, cameras, root, initial, loss, loss_scale, max_steps, max_cg_iterations, cg_tolerance,
                 step_tolerance);
    Tensor rotations = alloc(pairs, at::kDouble, {cameras, 3, 3});
    Tensor registered = alloc(pairs, at::kByte, {cameras});
    Tensor level = alloc(pairs, at::kInt, {cameras});
    Tensor residual = alloc(pairs, at::kDouble, {pairs.sym_size(0)});
    Tensor info = alloc(pairs, at::kLong, {kRotavgInfoWords});
    if (meta) return {rotations, registered, level, residual, info};
    const int64_t Q = pairs.size(0);
    const int64_t bytes = sfm_average_rotations_workspace_bytes(cameras, Q);
    TORCH_CHECK(bytes >= 0, "sfm_hip: average_rotations: ", cameras, " cameras, ", Q, " edges exceed the limits");
    Tensor ws = at::empty({bytes}, like(pairs, at::kByte));
    const sfm_rotavg_options options{(int32_t)loss, given ? SFM_ROTAVG_INIT_GIVEN : SFM_ROTAVG_INIT_TREE, (int32_t)max_steps,
                                     (int32_t)max_cg_iterations, loss_scale, cg_tolerance, step_tolerance};
    ok(sfm_average_rotations(cameras, Q, ptr<int32_t>(pairs), ptr<double>(relative), ptr<double>(weights), root,
                             given ? ptr<double>(*initial) : nullptr, &options, ptr<double>(rotations), ptr<uint8_t>(registered),
                             ptr<int32_t>(level), ptr<double>(residual), reinterpret_cast<sfm_rotavg_info*>(ptr<int64_t>(info)), ws.data_ptr(), bytes,
                             current_stream()),
       "sfm_average_rotations");
    return {rotations, registered, level, residual, info};
}

// translation averaging over a view graph (sfm_translation_averaging.hip): pairs int32 [Q, 2], directions f64 [Q, 3] (the
// world directions v_q, or with `rotations` f64 [C, 9] or [C, 3, 3] the pairs' t_q), weights f64 [Q], `cameras` = C, the root,
// initial f64 [C, 3] (given: the start; None: the spanning tree), the loss (SFM_BUNDLE_LOSS_*) with its scale (a sine) and the
// limits -> positions f64 [C, 3], registered uint8 [C], level int32 [C] (-1: unregistered), residual f64 [Q] (radians),
// scale f64 [Q], info int64 [5] viewing the sfm_transavg_info record.  The call synchronises the stream.
constexpr int64_t kTransavgInfoWords = sizeof(sfm_transavg_info) / 8;

void transavg_check(const Tensor& pairs, const Tensor& directions, const std::optional<Tensor>& rotations, const Tensor& weights,
                    int64_t cameras, int64_t root, const std::optional<Tensor>& initial, int64_t loss, double loss_scale,
                    int64_t warmup_steps, int64_t max_steps, int64_t max_cg_iterations, double cg_tolerance,
                    double step_tolerance) {
    graph_solver_check("average_translations", pairs, weights, cameras, root, loss, loss_scale, max_steps, max_cg_iterations,
                       cg_tolerance, step_tolerance);
    TORCH_CHECK(directions.dim() == 2 && directions.size(0) == pairs.size(0) && directions.size(1) == 3,
                "sfm_hip: directions must be [Q, 3]");
    if (rotations.has_value() && rotations->defined()) rotation_table_check(*rotations, cameras, "rotations", "cameras");
    if (initial.has_value() && initial->defined())
        TORCH_CHECK(initial->dim() == 2 && initial->size(0) == cameras && initial->size(1) == 3, "sfm_hip: initial must be [cameras, 3]");
    TORCH_CHECK(warmup_steps >= 0 && warmup_steps <= 0x7FFFFFFF, "sfm_hip: warmup_steps must be in [0, 2^31)");
}

using TransavgResult = std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>;

TransavgResult average_translations_new(bool meta, const Tensor& pairs, const Tensor& directions, const std::optional<Tensor>& rotations,
                                        const Tensor& weights, int64_t cameras, int64_t root, const std::optional<Tensor>& initial,
                                        int64_t loss, double loss_scale, int64_t warmup_steps, int64_t max_steps,
                                        int64_t max_cg_iterations, double cg_tolerance, double step_tolerance) {
    const OpDevice scope(pairs, meta);
    const bool rotated = rotations.has_value() && rotations->defined();
    const bool given = initial.has_value() && initial->defined();
    if (!meta) {
        need(pairs, "pairs", at::kInt);
        need(directions, "directions", at::kDouble);
        need(weights, "weights", at::kDouble);
        if (rotated) need(*rotations, "rotations", at::kDouble);
        if (given) need(*initial, "initial", at::kDouble);
    }
    transavg_check(pairs, directions, rotations, weights, cameras, root, initial, loss, loss_scale, warmup_steps, max_steps,
                   max_cg_iterations, cg_tolerance, step_tolerance);
    Tensor positions = alloc(pairs, at::kDouble, {cameras, 3});
    Tensor registered = alloc(pairs, at::kByte, {cameras});
    Tensor level = alloc(pairs, at::kInt, {cameras});
    Tensor residual = alloc(pairs, at::kDouble, {pairs.sym_size(0)});
    Tensor scale = alloc(pairs, at::kDouble, {pairs.sym_size(0)});
    Tensor info = alloc(pairs, at::kLong, {kTransavgInfoWords});
    if (meta) return {positions, registered, level, residual, scale, info};
    const int64_t Q = pairs.size(0);
    const int64_t bytes = sfm_average_translations_workspace_bytes(cameras, Q);
    TORCH_CHECK(bytes >= 0, "sfm_hip: average_translations: ", cameras, " cameras, ", Q, " edges exceed the limits");
    Tensor ws = at::empty({bytes}, like(pairs, at::kByte));
    const sfm_transavg_options options{(int32_t)loss, given ? SFM_TRANSAVG_INIT_GIVEN : SFM_TRANSAVG_INIT_TREE, (int32_t)max_steps,
                                       (int32_t)max_cg_iterations, (int32_t)warmup_steps, 0, loss_scale, cg_tolerance,
                                       step_tolerance};
    ok(sfm_average_translations(cameras, Q, ptr<int32_t>(pairs), ptr<double>(directions),
                                rotated ? ptr<double>(*rotations) : nullptr, ptr<double>(weights), root,
                                given ? ptr<double>(*initial) : nullptr, &options, ptr<double>(positions),
                                ptr<uint8_t>(registered), ptr<int32_t>(level), ptr<double>(residual), ptr<double>(scale),
                                reinterpret_cast<sfm_transavg_info*>(ptr<int64_t>(info)), ws.data_ptr(), bytes, current_stream()),
       "sfm_average_translations");
    return {positions, registered, level, residual, scale, info};
}
}  // namespace

// the C-ABI version this op library was compiled against (include/sfm_hip.h); ops.load() compares it with the
// libsfm_hip.so it finds next to it
extern "C" int sfm_torch_ops_abi_version(void) { return SFM_ABI_VERSION; }

TORCH_LIBRARY(sfm_hip, m) {
    m.def("normalize_coords(Tensor pix_a, Tensor pix_b, float fx, float fy, float cx, float cy) -> Tensor");
    m.def("normalize_coords_(Tensor pix_a, Tensor pix_b, float fx, float fy, float cx, float cy, Tensor(a!) out) -> ()");
    m.def("sample_philox(int seed, int seed_stride, int h_begin, int h_count, int n, int batch, Device device) -> Tensor");
    m.def("fit_eight_point(Tensor corr, Tensor S) -> (Tensor, Tensor)");
    m.def("fit_eight_point_(Tensor corr, Tensor S, Tensor(a!) E, Tensor(b!) flags) -> ()");
    m.def("sample_fit_philox_(Tensor corr, int seed, Tensor? seed_dev, int seed_stride, int h_begin, Tensor(a!) S, "
          "Tensor(b!) E, Tensor(c!) flags) -> ()");
    m.def("score_sed(Tensor corr, Tensor E, Tensor S, float thr, bool exact=False) -> (Tensor, Tensor, Tensor)");
    m.def("score_sed_(Tensor corr, Tensor E, Tensor S, float thr, Tensor(a!) cnt, Tensor(b!) s1, Tensor(c!) s2, "
          "Tensor(d!)? workspace) -> ()");
    m.def("ransac_pass_small_(Tensor corr, int seed, Tensor? seed_dev, bool use_philox, int h_begin, float thr, "
          "float min_extra, int aggregation, int h_offset, Tensor(a!) S, Tensor(b!) E, Tensor(c!) flags, Tensor(d!) cnt, "
          "Tensor(e!) s1, Tensor(f!) s2, Tensor(g!) result, Tensor(h!)? mask, Tensor(i!) workspace) -> ()");
    m.def("ransac_pass_large_(Tensor corr, int seed, Tensor? seed_dev, bool use_philox, int h_begin, float thr, "
          "float min_extra, int aggregation, int h_offset, Tensor(a!) S, Tensor(b!) E, Tensor(c!) flags, Tensor(d!) cnt, "
          "Tensor(e!) s1, Tensor(f!) s2, Tensor(g!) result, Tensor(h!)? mask, Tensor(i!) workspace) -> ()");
    m.def("select_best(Tensor cnt, Tensor s1, Tensor s2, Tensor? flags, float min_extra, int aggregation, "
          "int h_offset=0, int sample_size=8) -> Tensor");
    m.def("select_best_(Tensor cnt, Tensor s1, Tensor s2, Tensor? flags, float min_extra, int aggregation, "
          "int h_offset, Tensor(a!) result, int sample_size=8) -> ()");
    m.def("inlier_mask(Tensor corr, Tensor E, Tensor S, Tensor result, float thr, int sample_size=8) -> Tensor");
    m.def("inlier_mask_(Tensor corr, Tensor E, Tensor S, Tensor result, float thr, Tensor(a!) mask, int sample_size=8) -> ()");
    m.def("cheirality(Tensor corr, Tensor pose_rt, float distance_threshold) -> Tensor");
    m.def("triangulate(Tensor corr, Tensor P1, Tensor P2) -> Tensor");
    m.def("five_point_fit(Tensor corr, Tensor S) -> (Tensor, Tensor)");
    m.def("five_point_fit_(Tensor corr, Tensor S, Tensor(a!) E, Tensor(b!) flags) -> ()");
    m.def("five_point_ransac_pass_(Tensor corr, int seed, int seed_stride, bool use_philox, int h_begin, float thr, float min_extra, "
          "int aggregation, Tensor(a!) S, Tensor(b!) E, Tensor(c!) flags, Tensor(d!) cnt, Tensor(e!) s1, Tensor(f!) s2, "
          "Tensor(g!) result, Tensor(h!)? mask) -> ()");
    m.def("homography_fit(Tensor corr, Tensor S) -> (Tensor, Tensor)");
    m.def("homography_score(Tensor corr, Tensor H, Tensor S, float thr) -> (Tensor, Tensor, Tensor)");
    m.def("homography_inlier_mask(Tensor corr, Tensor H, Tensor S, Tensor result, float thr) -> Tensor");
    m.def("homography_ransac_pass_(Tensor corr, int seed, int seed_stride, bool use_philox, int h_begin, float thr, float min_extra, "
          "int aggregation, Tensor(a!) S, Tensor(b!) H, Tensor(c!) flags, Tensor(d!) cnt, Tensor(e!) s1, Tensor(f!) s2, "
          "Tensor(g!) result, Tensor(h!)? mask) -> ()");
    m.def("verify_pairs_(Tensor corr, Tensor offset, Tensor min_extra, int seed, int seed_stride, int h_begin, float thr, int aggregation, "
          "float max_ratio, Tensor(a!) S, Tensor(b!) H, Tensor(c!) E, Tensor(d!) h_flags, Tensor(e!) h_cnt, Tensor(f!) h_s1, "
          "Tensor(g!) h_s2, Tensor(h!) e_flags, Tensor(i!) e_cnt, Tensor(j!) e_s1, Tensor(k!) e_s2, Tensor(l!) h_result, "
          "Tensor(m!) e_result, Tensor(n!) h_mask, Tensor(o!) e_mask, Tensor(p!) verdict) -> ()");
    m.def("pair_poses(Tensor corr, Tensor offset, Tensor E, Tensor e_result, Tensor e_mask, Tensor verdict, "
          "float distance_threshold) -> (Tensor, Tensor)");
    m.def("refine_pair_poses(Tensor corr, Tensor offset, Tensor pose, float thr, int aggregation, int rounds, int max_steps) -> "
          "(Tensor, Tensor, Tensor)");
    m.def("pnp_fit(Tensor pts, Tensor S, float[] K) -> (Tensor, Tensor)");
    m.def("pnp_fit_(Tensor pts, Tensor S, float[] K, Tensor(a!) model, Tensor(b!) flags) -> ()");
    m.def("p3p_fit(Tensor pts, Tensor S, float[] K) -> (Tensor, Tensor)");
    m.def("p3p_fit_(Tensor pts, Tensor S, float[] K, Tensor(a!) model, Tensor(b!) flags) -> ()");
    m.def("pnp_score(Tensor pts, Tensor model, Tensor S, float[] K, float thr, int sample_size=6) -> (Tensor, Tensor, Tensor)");
    m.def("pnp_score_(Tensor pts, Tensor model, Tensor S, float[] K, float thr, Tensor(a!) cnt, Tensor(b!) s1, "
          "Tensor(c!) s2, int sample_size=6) -> ()");
    m.def("pnp_ransac_pass_(Tensor pts, int seed, int seed_stride, bool use_philox, int h_begin, float[] K, float thr, "
          "float min_extra, int aggregation, Tensor(a!) S, Tensor(b!) model, Tensor(c!) flags, Tensor(d!) cnt, Tensor(e!) s1, "
          "Tensor(f!) s2, Tensor(g!) result, Tensor(h!)? mask) -> ()");
    m.def("p3p_ransac_pass_(Tensor pts, int seed, int seed_stride, bool use_philox, int h_begin, float[] K, float thr, "
          "float min_extra, int aggregation, Tensor(a!) S, Tensor(b!) model, Tensor(c!) flags, Tensor(d!) cnt, Tensor(e!) s1, "
          "Tensor(f!) s2, Tensor(g!) result, Tensor(h!)? mask) -> ()");
    m.def("pnp_refine(Tensor pts, Tensor model, Tensor mask, Tensor err, float[] K, float thr, int aggregation, int rounds, "
          "int max_steps) -> (Tensor, Tensor, Tensor)");
    m.def("pnp_refine_(Tensor pts, Tensor model, Tensor mask, Tensor err, float[] K, float thr, int aggregation, int rounds, "
          "int max_steps, Tensor(a!) model_out, Tensor(b!) mask_out, Tensor(c!) info) -> ()");
    m.def("register_views(Tensor pts, Tensor offset, Tensor min_extra, float[] K, int seed, int seed_stride, int h_begin, int h, "
          "float thr, int aggregation, int refine_rounds, int refine_max_steps) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("register_views_(Tensor pts, Tensor offset, Tensor min_extra, float[] K, int seed, int seed_stride, int h_begin, float thr, "
          "int aggregation, int refine_rounds, int refine_max_steps, Tensor(a!) S, Tensor(b!) model, Tensor(c!) flags, Tensor(d!) cnt, "
          "Tensor(e!) s1, Tensor(f!) s2, Tensor(g!) result, Tensor(h!) mask, Tensor(i!) pose_out, Tensor(j!) mask_out, "
          "Tensor(k!) info, Tensor(l!) status) -> ()");
    m.def("similarity_ransac_pass(Tensor pairs, int seed, int seed_stride, int h_begin, int h, float thr, float min_extra, "
          "int aggregation) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("similarity_ransac_pass_(Tensor pairs, int seed, int seed_stride, bool use_philox, int h_begin, float thr, float min_extra, "
          "int aggregation, Tensor(a!) S, Tensor(b!) model, Tensor(c!) flags, Tensor(d!) cnt, Tensor(e!) s1, Tensor(f!) s2, "
          "Tensor(g!) result, Tensor(h!)? mask) -> ()");
    m.def("similarity_fit(Tensor pairs, Tensor? mask) -> (Tensor, Tensor)");
    m.def("similarity_fit_(Tensor pairs, Tensor? mask, Tensor(a!) model_out, Tensor(b!) flags_out) -> ()");
    m.def("similarity_refine(Tensor pairs, Tensor model, Tensor mask, Tensor err, float thr, int aggregation, int rounds) -> "
          "(Tensor, Tensor, Tensor)");
    m.def("similarity_refine_(Tensor pairs, Tensor model, Tensor mask, Tensor err, float thr, int aggregation, int rounds, "
          "Tensor(a!) model_out, Tensor(b!) mask_out, Tensor(c!) info) -> ()");
    m.def("align_models(Tensor pairs, Tensor offset, Tensor thr, Tensor min_extra, int max_items, int seed, int seed_stride, "
          "int h_begin, int h, int aggregation, int refine_rounds) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("align_models_(Tensor pairs, Tensor offset, Tensor thr, Tensor min_extra, int max_items, int seed, int seed_stride, "
          "int h_begin, int aggregation, int refine_rounds, Tensor(a!) S, Tensor(b!) model, Tensor(c!) flags, Tensor(d!) cnt, "
          "Tensor(e!) s1, Tensor(f!) s2, Tensor(g!) result, Tensor(h!) mask, Tensor(i!) model_out, Tensor(j!) mask_out, "
          "Tensor(k!) info, Tensor(l!) status) -> ()");
    m.def("plane_sweep(Tensor images, Tensor K, Tensor poses, Tensor refs, Tensor sources, Tensor depths, int radius, int top_k, "
          "int min_sources, float min_variance, bool return_volume) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("plane_sweep_(Tensor images, Tensor K, Tensor poses, Tensor refs, Tensor sources, Tensor depths, int radius, int top_k, "
          "int min_sources, float min_variance, Tensor(a!) depth, Tensor(b!) index, Tensor(c!) cost, Tensor(d!) status, "
          "Tensor(e!)? volume) -> ()");
    m.def("filter_depth_maps(Tensor depth, Tensor K, Tensor poses, Tensor refs, Tensor sources, float max_pixel_error, "
          "float max_relative_depth_error, int min_consistent) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("filter_depth_maps_(Tensor depth, Tensor K, Tensor poses, Tensor refs, Tensor sources, float max_pixel_error, "
          "float max_relative_depth_error, int min_consistent, Tensor(a!) count, Tensor(b!) filtered, Tensor(c!) points, "
          "Tensor(d!) status) -> ()");
    m.def("sgm_aggregate(Tensor volume, Tensor depths, float p1, float p2, float invalid_cost, int paths, bool return_aggregated) -> "
          "(Tensor, Tensor, Tensor, Tensor)");
    m.def("sgm_aggregate_(Tensor volume, Tensor depths, float p1, float p2, float invalid_cost, int paths, Tensor(a!) depth, "
          "Tensor(b!) index, Tensor(c!) cost, Tensor(d!)? aggregated) -> ()");
    m.def("tsdf_integrate(Tensor sum,Tensor count, Tensor? grey_sum, Tensor depth, Tensor? images, Tensor K, Tensor poses, Tensor views, "
          "float ox, float oy, float oz, float voxel_size, float truncation) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("tsdf_integrate_(Tensor(a!) sum, Tensor(b!) count, Tensor(c!)? grey_sum, Tensor depth, Tensor? images, Tensor K, Tensor poses, "
          "Tensor views, float ox, float oy, float oz, float voxel_size, float truncation, Tensor(d!) status) -> ()");
    m.def("tsdf_extract_mesh(Tensor sum, Tensor count, Tensor? grey_sum, float ox, float oy, float oz, float voxel_size, int min_count, "
          "int max_triangles) -> (Tensor, Tensor, Tensor)");
    m.def("tsdf_extract_mesh_(Tensor sum, Tensor count, Tensor? grey_sum, float ox, float oy, float oz, float voxel_size, int min_count, "
          "Tensor(a!) vertices, Tensor(b!)? grey, Tensor(c!) total) -> ()");
    m.def("bundle_adjust(Tensor poses, Tensor points, Tensor camera_indices, Tensor point_indices, Tensor pixels, float[] K, "
          "int[] fixed, int max_steps) -> (Tensor, Tensor, Tensor)");
    m.def("bundle_adjust_(Tensor(a!) poses, Tensor(b!) points, Tensor camera_indices, Tensor point_indices, Tensor pixels, "
          "float[] K, int[] fixed, int max_steps, Tensor(c!) info) -> ()");
    m.def("bundle_adjust_pcg(Tensor poses, Tensor points, Tensor camera_indices, Tensor point_indices, Tensor pixels, "
          "float[] K, int[] fixed, int max_steps, int max_cg_iterations, float cg_tolerance) -> (Tensor, Tensor, Tensor)");
    m.def("bundle_adjust_pcg_(Tensor(a!) poses, Tensor(b!) points, Tensor camera_indices, Tensor point_indices, "
          "Tensor pixels, float[] K, int[] fixed, int max_steps, int max_cg_iterations, float cg_tolerance, "
          "Tensor(c!) info) -> ()");
    m.def("bundle_adjust_robust(Tensor poses, Tensor points, Tensor camera_indices, Tensor point_indices, Tensor pixels, "
          "float[] K, int[] fixed, int max_steps, int loss, float loss_scale) -> (Tensor, Tensor, Tensor)");
    m.def("bundle_adjust_robust_(Tensor(a!) poses, Tensor(b!) points, Tensor camera_indices, Tensor point_indices, "
          "Tensor pixels, float[] K, int[] fixed, int max_steps, int loss, float loss_scale, Tensor(c!) info) -> ()");
    m.def("bundle_adjust_pcg_robust(Tensor poses, Tensor points, Tensor camera_indices, Tensor point_indices, Tensor pixels, "
          "float[] K, int[] fixed, int max_steps, int max_cg_iterations, float cg_tolerance, int loss, float loss_scale) -> "
          "(Tensor, Tensor, Tensor)");
    m.def("bundle_adjust_pcg_robust_(Tensor(a!) poses, Tensor(b!) points, Tensor camera_indices, Tensor point_indices, "
          "Tensor pixels, float[] K, int[] fixed, int max_steps, int max_cg_iterations, float cg_tolerance, int loss, "
          "float loss_scale, Tensor(c!) info) -> ()");
    m.def("bundle_adjust_calibrated(Tensor poses, Tensor points, Tensor camera_indices, Tensor point_indices, Tensor pixels, "
          "float[] K, int[] fixed, int max_steps, int loss, float loss_scale, int refine) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("bundle_adjust_calibrated_(Tensor(a!) poses, Tensor(b!) points, Tensor camera_indices, Tensor point_indices, "
          "Tensor pixels, float[] K, int[] fixed, int max_steps, int loss, float loss_scale, int refine, Tensor(c!) info, "
          "Tensor(d!) K_out) -> ()");
    m.def("triangulate_tracks(Tensor poses, Tensor camera_indices, Tensor point_indices, Tensor pixels, int points, float[] K, "
          "int min_views, float min_angle, float max_error, int refine_steps) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("triangulate_tracks_(Tensor poses, Tensor camera_indices, Tensor point_indices, Tensor pixels, int points, "
          "float[] K, int min_views, float min_angle, float max_error, int refine_steps, Tensor(a!) points_out, "
          "Tensor(b!) status, Tensor(c!) obs_error, Tensor(d!) angle, Tensor(e!) info) -> ()");
    m.def("build_tracks(Tensor image_offset, Tensor pair_images, Tensor match_offset, Tensor match_index, int features) -> "
          "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("build_tracks_(Tensor image_offset, Tensor pair_images, Tensor match_offset, Tensor match_index, int features, "
          "Tensor(a!) component, Tensor(b!) track, Tensor(c!) status, Tensor(d!) camera_index, Tensor(e!) point_index, "
          "Tensor(f!) feature_index, Tensor(g!) info) -> ()");
    m.def("average_rotations(Tensor pairs, Tensor relative, Tensor weights, int cameras, int root, Tensor? initial, int loss, "
          "float loss_scale, int max_steps, int max_cg_iterations, float cg_tolerance, float step_tolerance) -> "
          "(Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("average_translations(Tensor pairs, Tensor directions, Tensor? rotations, Tensor weights, int cameras, int root, "
          "Tensor? initial, int loss, float loss_scale, int warmup_steps, int max_steps, int max_cg_iterations, "
          "float cg_tolerance, float step_tolerance) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
}

// ROCm devices dispatch under torch's "CUDA" key (the name of the dispatch key, not a CUDA code path)
TORCH_LIBRARY_IMPL(sfm_hip, CUDA, m) {
    m.impl("normalize_coords", &Forms<&normalize_coords_new>::call<false>);
    m.impl("normalize_coords_", &normalize_coords_out);
    m.impl("fit_eight_point", &Forms<&essential_fit_new<fit_eight_point_out>>::call<false>);
    m.impl("five_point_fit", &Forms<&essential_fit_new<five_point_fit_out>>::call<false>);
    m.impl("five_point_fit_", &five_point_fit_out);
    m.impl("five_point_ransac_pass_", &five_point_ransac_pass_out);
    m.impl("fit_eight_point_", &fit_eight_point_out);
    m.impl("sample_fit_philox_", &sample_fit_philox_out);
    m.impl("score_sed", &Forms<&score_sed_new>::call<false>);
    m.impl("score_sed_", &score_sed_out);
    m.impl("ransac_pass_small_", &ransac_pass_small_out);
    m.impl("ransac_pass_large_", &ransac_pass_large_out);
    m.impl("select_best", &Forms<&select_best_new>::call<false>);
    m.impl("select_best_", &select_best_out);
    m.impl("inlier_mask", &Forms<&inlier_mask_new>::call<false>);
    m.impl("inlier_mask_", &inlier_mask_out);
    m.impl("cheirality", &Forms<&cheirality_new>::call<false>);
    m.impl("triangulate", &Forms<&triangulate_new>::call<false>);
    m.impl("homography_fit", &Forms<&essential_fit_new<homography_fit_out>>::call<false>);
    m.impl("homography_score", &Forms<&homography_score_new>::call<false>);
    m.impl("homography_inlier_mask", &Forms<&homography_inlier_mask_new>::call<false>);
    m.impl("homography_ransac_pass_", &homography_ransac_pass_out);
    m.impl("verify_pairs_", &verify_pairs_out);
    m.impl("pair_poses", &Forms<&pair_poses_new>::call<false>);
    m.impl("refine_pair_poses", &Forms<&refine_pair_poses_new>::call<false>);
    m.impl("pnp_fit", &Forms<&pose_fit_new<pnp_fit_out>>::call<false>);
    m.impl("pnp_fit_", &pnp_fit_out);
    m.impl("pnp_score", &Forms<&pnp_score_new>::call<false>);
    m.impl("pnp_score_", &pnp_score_out);
    m.impl("pnp_ransac_pass_", &pnp_ransac_pass_out);
    m.impl("p3p_fit", &Forms<&pose_fit_new<p3p_fit_out>>::call<false>);
    m.impl("p3p_fit_", &p3p_fit_out);
    m.impl("p3p_ransac_pass_", &p3p_ransac_pass_out);
    m.impl("pnp_refine", &Forms<&pnp_refine_new>::call<false>);
    m.impl("pnp_refine_", &pnp_refine_out);
    m.impl("register_views", &Forms<&register_views_new>::call<false>);
    m.impl("register_views_", &register_views_out);
    m.impl("similarity_ransac_pass", &Forms<&similarity_ransac_pass_new>::call<false>);
    m.impl("similarity_ransac_pass_", &similarity_ransac_pass_out);
    m.impl("similarity_fit", &Forms<&similarity_fit_new>::call<false>);
    m.impl("similarity_fit_", &similarity_fit_out);
    m.impl("similarity_refine", &Forms<&similarity_refine_new>::call<false>);
    m.impl("similarity_refine_", &similarity_refine_out);
    m.impl("align_models", &Forms<&align_models_new>::call<false>);
    m.impl("align_models_", &align_models_out);
    m.impl("plane_sweep", &Forms<&plane_sweep_new>::call<false>);
    m.impl("plane_sweep_", &plane_sweep_out);
    m.impl("filter_depth_maps", &Forms<&filter_depth_maps_new>::call<false>);
    m.impl("filter_depth_maps_", &filter_depth_maps_out);
    m.impl("sgm_aggregate", &Forms<&sgm_aggregate_new>::call<false>);
    m.impl("sgm_aggregate_", &sgm_aggregate_out);
    m.impl("tsdf_integrate", &Forms<&tsdf_integrate_new>::call<false>);
    m.impl("tsdf_integrate_", &tsdf_integrate_out);
    m.impl("tsdf_extract_mesh", &Forms<&tsdf_extract_mesh_new>::call<false>);
    m.impl("tsdf_extract_mesh_", &tsdf_extract_mesh_out);
    m.impl("bundle_adjust", &Forms<&bundle_adjust_new>::call<false>);
    m.impl("bundle_adjust_", &bundle_adjust_out);
    m.impl("bundle_adjust_pcg", &Forms<&bundle_adjust_pcg_new>::call<false>);
    m.impl("bundle_adjust_pcg_", &bundle_adjust_pcg_out);
    m.impl("bundle_adjust_robust", &Forms<&bundle_adjust_robust_new>::call<false>);
    m.impl("bundle_adjust_robust_", &bundle_adjust_robust_out);
    m.impl("bundle_adjust_pcg_robust", &Forms<&bundle_adjust_pcg_robust_new>::call<false>);
    m.impl("bundle_adjust_pcg_robust_", &bundle_adjust_pcg_robust_out);
    m.impl("bundle_adjust_calibrated", &Forms<&bundle_calibrated_new>::call<false>);
    m.impl("bundle_adjust_calibrated_", &bundle_adjust_calibrated_out);
    m.impl("triangulate_tracks", &Forms<&triangulate_tracks_new>::call<false>);
    m.impl("triangulate_tracks_", &triangulate_tracks_out);
    m.impl("build_tracks", &Forms<&build_tracks_new>::call<false>);
    m.impl("build_tracks_", &build_tracks_out);
    m.impl("average_rotations", &Forms<&average_rotations_new>::call<false>);
    m.impl("average_translations", &Forms<&average_translations_new>::call<false>);
}

// sample_philox has no tensor argument to dispatch on: registered for every backend, it checks its device itself
TORCH_LIBRARY_IMPL(sfm_hip, CompositeExplicitAutograd, m) { m.impl("sample_philox", &sample_philox); }

// Under fake tensors a functional form gives its outputs' shapes; an in-place form has nothing to compute
TORCH_LIBRARY_IMPL(sfm_hip, Meta, m) {
    m.impl("normalize_coords", &Forms<&normalize_coords_new>::call<true>);
    m.impl("normalize_coords_", &Noop<&normalize_coords_out>::call);
    m.impl("fit_eight_point", &Forms<&essential_fit_new<fit_eight_point_out>>::call<true>);
    m.impl("five_point_fit", &Forms<&essential_fit_new<five_point_fit_out>>::call<true>);
    m.impl("five_point_fit_", &Noop<&five_point_fit_out>::call);
    m.impl("five_point_ransac_pass_", &Noop<&five_point_ransac_pass_out>::call);
    m.impl("fit_eight_point_", &Noop<&fit_eight_point_out>::call);
    m.impl("sample_fit_philox_", &Noop<&sample_fit_philox_out>::call);
    m.impl("score_sed", &Forms<&score_sed_new>::call<true>);
    m.impl("score_sed_", &Noop<&score_sed_out>::call);
    m.impl("ransac_pass_small_", &Noop<&ransac_pass_small_out>::call);
    m.impl("ransac_pass_large_", &Noop<&ransac_pass_large_out>::call);
    m.impl("select_best", &Forms<&select_best_new>::call<true>);
    m.impl("select_best_", &Noop<&select_best_out>::call);
    m.impl("inlier_mask", &Forms<&inlier_mask_new>::call<true>);
    m.impl("inlier_mask_", &Noop<&inlier_mask_out>::call);
    m.impl("cheirality", &Forms<&cheirality_new>::call<true>);
    m.impl("triangulate", &Forms<&triangulate_new>::call<true>);
    m.impl("homography_fit", &Forms<&essential_fit_new<homography_fit_out>>::call<true>);
    m.impl("homography_score", &Forms<&homography_score_new>::call<true>);
    m.impl("homography_inlier_mask", &Forms<&homography_inlier_mask_new>::call<true>);
    m.impl("homography_ransac_pass_", &Noop<&homography_ransac_pass_out>::call);
    m.impl("verify_pairs_", &Noop<&verify_pairs_out>::call);
    m.impl("pair_poses", &Forms<&pair_poses_new>::call<true>);
    m.impl("refine_pair_poses", &Forms<&refine_pair_poses_new>::call<true>);
    m.impl("pnp_fit", &Forms<&pose_fit_new<pnp_fit_out>>::call<true>);
    m.impl("pnp_fit_", &Noop<&pnp_fit_out>::call);
    m.impl("pnp_score", &Forms<&pnp_score_new>::call<true>);
    m.impl("pnp_score_", &Noop<&pnp_score_out>::call);
    m.impl("pnp_ransac_pass_", &Noop<&pnp_ransac_pass_out>::call);
    m.impl("p3p_fit", &Forms<&pose_fit_new<p3p_fit_out>>::call<true>);
    m.impl("p3p_fit_", &Noop<&p3p_fit_out>::call);
    m.impl("p3p_ransac_pass_", &Noop<&p3p_ransac_pass_out>::call);
    m.impl("pnp_refine", &Forms<&pnp_refine_new>::call<true>);
    m.impl("pnp_refine_", &Noop<&pnp_refine_out>::call);
    m.impl("register_views", &Forms<&register_views_new>::call<true>);
    m.impl("register_views_", &Noop<&register_views_out>::call);
    m.impl("similarity_ransac_pass", &Forms<&similarity_ransac_pass_new>::call<true>);
    m.impl("similarity_ransac_pass_", &Noop<&similarity_ransac_pass_out>::call);
    m.impl("similarity_fit", &Forms<&similarity_fit_new>::call<true>);
    m.impl("similarity_fit_", &Noop<&similarity_fit_out>::call);
    m.impl("similarity_refine", &Forms<&similarity_refine_new>::call<true>);
    m.impl("similarity_refine_", &Noop<&similarity_refine_out>::call);
    m.impl("align_models", &Forms<&align_models_new>::call<true>);
    m.impl("align_models_", &Noop<&align_models_out>::call);
    m.impl("plane_sweep", &Forms<&plane_sweep_new>::call<true>);
    m.impl("plane_sweep_", &Noop<&plane_sweep_out>::call);
    m.impl("filter_depth_maps", &Forms<&filter_depth_maps_new>::call<true>);
    m.impl("filter_depth_maps_", &Noop<&filter_depth_maps_out>::call);
    m.impl("sgm_aggregate", &Forms<&sgm_aggregate_new>::call<true>);
    m.impl("sgm_aggregate_", &Noop<&sgm_aggregate_out>::call);
    m.impl("tsdf_integrate", &Forms<&tsdf_integrate_new>::call<true>);
    m.impl("tsdf_integrate_", &Noop<&tsdf_integrate_out>::call);
    m.impl("tsdf_extract_mesh", &Forms<&tsdf_extract_mesh_new>::call<true>);
    m.impl("tsdf_extract_mesh_", &Noop<&tsdf_extract_mesh_out>::call);
    m.impl("bundle_adjust", &Forms<&bundle_adjust_new>::call<true>);
    m.impl("bundle_adjust_", &Noop<&bundle_adjust_out>::call);
    m.impl("bundle_adjust_pcg", &Forms<&bundle_adjust_pcg_new>::call<true>);
    m.impl("bundle_adjust_pcg_", &Noop<&bundle_adjust_pcg_out>::call);
    m.impl("bundle_adjust_robust", &Forms<&bundle_adjust_robust_new>::call<true>);
    m.impl("bundle_adjust_robust_", &Noop<&bundle_adjust_robust_out>::call);
    m.impl("bundle_adjust_pcg_robust", &Forms<&bundle_adjust_pcg_robust_new>::call<true>);
    m.impl("bundle_adjust_pcg_robust_", &Noop<&bundle_adjust_pcg_robust_out>::call);
    m.impl("bundle_adjust_calibrated", &Forms<&bundle_calibrated_new>::call<true>);
    m.impl("bundle_adjust_calibrated_", &Noop<&bundle_adjust_calibrated_out>::call);
    m.impl("triangulate_tracks", &Forms<&triangulate_tracks_new>::call<true>);
    m.impl("triangulate_tracks_", &Noop<&triangulate_tracks_out>::call);
    m.impl("build_tracks", &Forms<&build_tracks_new>::call<true>);
    m.impl("build_tracks_", &Noop<&build_tracks_out>::call);
    m.impl("average_rotations", &Forms<&average_rotations_new>::call<true>);
    m.impl("average_translations", &Forms<&average_translations_new>::call<true>);
}
