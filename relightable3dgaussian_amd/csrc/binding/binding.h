// binding.h -- what the operator families of the `_C` binding share: how a tensor becomes a pointer
// the C ABI (include/r3dg_hip.h) may read, which device and stream a call runs on, and where the
// library's scratch memory comes from. There is no CPU path and the kernels check no pointer, so a
// host or foreign-device tensor must be refused here, before any HIP call.
//
// Every data_ptr that reaches an r3dg_* call comes from one of Call's accessors or from a tensor
// the binding itself has just allocated on the call's device.
#pragma once
#include <torch/extension.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>

#include <map>
#include <optional>
#include <string>
#include <tuple>
#include <vector>

#include "r3dg_hip.h"

namespace binding {

using torch::Tensor;

// errors from the C ABI surface as RuntimeError with the library's message
inline void check(int rc, const char* what) {
    if (rc != R3DG_OK) throw std::runtime_error(std::string(what) + ": " + r3dg_last_error());
}

inline const char* dtype_name(torch::ScalarType t) {
    return t == torch::kFloat32 ? "float32"
           : t == torch::kInt32 ? "int32"
           : t == torch::kUInt8 ? "uint8"
                                : c10::toString(t);
}

// One per binding call, built from the call's anchor tensor (means3D, base_color, param, ...) before
// any pointer is taken: the anchor must be on a GPU, its device is the call's device, and the device
// guard and the stream are that device's. Every other tensor of the call goes through one of three
// policies, each refusing with "<entry>: <argument> must be ...":
//   moved      float32, copied to the call's device if it is elsewhere, made contiguous, numel 0 =
//              absent. The reference's own surface only (its callers rely on the copy).
//   on_device  already on the call's device, of the given type, made contiguous if it is not.
//   in_place   already on the call's device, of the given type and contiguous: the kernel writes it
//              or the caller keeps its storage, so a contiguous copy would not do.
struct Call {
    const char* const who;
    const torch::Device dev;
    const c10::OptionalDeviceGuard guard;

    Call(const char* who, const Tensor& anchor, const char* name)
        : who(who), dev(gpu_of(who, anchor, name)), guard(dev) {}

    r3dg_stream_t stream() const { return (r3dg_stream_t)c10::hip::getCurrentHIPStream(dev.index()).stream(); }
    torch::TensorOptions options(torch::ScalarType type = torch::kFloat32) const {
        return torch::TensorOptions().dtype(type).device(dev);
    }

    // a float tensor must be float32 already; an integer one (the backward's radii) is converted to int32,
    // as the reference's surface does
    Tensor moved(const Tensor& t, const char* name, torch::ScalarType type = torch::kFloat32) const {
        if (t.numel() == 0) return t;
        const auto got = t.scalar_type();
        TORCH_CHECK(type == torch::kFloat32 ? got == type : c10::isIntegralType(got, false), who, ": ", name,
                    " must be ", dtype_name(type), ", got ", dtype_name(got));
        return t.to(dev, type).contiguous();
    }
    Tensor on_device(const Tensor& t, const char* name, torch::ScalarType type = torch::kFloat32) const {
        require(t, name, type);
        return t.contiguous();
    }
    template <class T = float>
    T* in_place(const Tensor& t, const char* name) const {
        require(t, name, c10::CppTypeToScalarType<T>::value);
        TORCH_CHECK(t.is_contiguous(), who, ": ", name,
                    " must be contiguous (it is written in place or its storage is kept)");
        return t.data_ptr<T>();
    }
    // index [G], int32 or int64 -> contiguous int32 on the call's device
    Tensor index(const Tensor& t, const char* name) const {
        TORCH_CHECK(t.dim() == 1 && (t.scalar_type() == torch::kInt32 || t.scalar_type() == torch::kInt64), who,
                    ": ", name, " must be a 1-D int32 or int64 tensor");
        require(t, name, t.scalar_type());
        return t.to(torch::kInt32).contiguous();
    }

    // the device and type check of on_device and in_place alone, for a tensor whose pointer is passed with
    // the tensor's own strides (activate_backward's column-block upstreams)
    void require(const Tensor& t, const char* name, torch::ScalarType type = torch::kFloat32) const {
        TORCH_CHECK(t.is_cuda() && t.device() == dev, who, ": ", name, " must be a GPU tensor on ", dev, ", got ",
                    t.device());
        TORCH_CHECK(t.scalar_type() == type, who, ": ", name, " must be ", dtype_name(type), ", got ",
                    dtype_name(t.scalar_type()));
    }

   private:
    static torch::Device gpu_of(const char* who, const Tensor& anchor, const char* name) {
        TORCH_CHECK(anchor.is_cuda(), who, ": ", name, " must be a GPU tensor (this build has no CPU path), got ",
                    anchor.device());
        return anchor.device();
    }
};

// a `moved` tensor's pointer; empty (numel 0) means absent, as the reference's data_ptr of an empty tensor
inline const float* opt_ptr(const Tensor& t) { return t.numel() == 0 ? nullptr : t.data_ptr<float>(); }

// The memory the library asks the caller for during one binding call: r3dg_alloc_fn is Scratch::alloc
// with a Scratch* as its context. Every block stays alive until the Scratch is destroyed at the end of
// the binding call, after the library has enqueued all of its kernels, so a library function may call
// its allocator any number of times (r3dg_bvh_trace_opacity does so twice when it sorts the rays). A
// block goes back to torch's caching allocator then, which is safe because that allocator is
// stream-ordered and the kernels were enqueued on the call's stream. Blocks the library hands back as
// results (densify_and_prune, trace_bvh) are found again with holder() and live on as tensors.
struct Scratch {
    const torch::TensorOptions bytes;  // uint8 on the call's device
    std::vector<Tensor> blocks;

    explicit Scratch(const Call& call) : bytes(call.options(torch::kUInt8)) {}

    static void* alloc(void* ctx, size_t nbytes) {
        auto* s = static_cast<Scratch*>(ctx);
        s->blocks.push_back(torch::empty({(int64_t)std::max<size_t>(nbytes, 256)}, s->bytes));
        return s->blocks.back().data_ptr();
    }
    // densify_and_prune's noise source, not scratch: n standard-normal floats from the device generator
    // (the reference's torch.normal), kept alive like a block
    static void* randn(void* ctx, size_t n) {
        auto* s = static_cast<Scratch*>(ctx);
        s->blocks.push_back(torch::randn({(int64_t)n}, s->bytes.dtype(torch::kFloat32)));
        return s->blocks.back().data_ptr();
    }
    // the block behind a pointer the library returned
    Tensor holder(const void* p, const char* who) const {
        for (const auto& b : blocks)
            if (b.data_ptr() == p) return b;
        TORCH_CHECK(false, who, ": the library returned memory it was not given");
        return Tensor();
    }
    // the one block of a context the library allocates from at most once (the forward's state buffers)
    Tensor buffer() const { return blocks.empty() ? torch::empty({0}, bytes) : blocks.back(); }
};

}  // namespace binding
