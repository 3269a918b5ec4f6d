// Device half of a batched handle, shared by batch.hip (with batch_structure.hip on its handle), gcw_batch.hip, cemp_batch.hip (with mpls_batch.hip on its handle), mst_batch.hip, refine_batch.hip, irls_batch.hip, lp_batch.hip, models_batch.hip and align_batch.hip: the device,
// one pooled stream, the arena of device blocks, the event pair around a timed launch, and the create wrapper of the C entry points.
// Host code only.  A batched call supplies its host validation, its kernels and its words for the refusals; the order of the
// refusals (nothing touches the device before open) and of the teardown is decided here.
#pragma once
#include <memory>
#include <type_traits>

#include "device_utils.h"

namespace desc {

struct BatchDevice {
    int device = 0;
    hipStream_t stream = nullptr;             // null until open() succeeds
    DevArena mem;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // timer_begin / timer_end: made at the first timed launch, kept for the handle's life
    double ms_structure = 0, ms_upload = 0;
    int64_t bytes_h2d = 0, bytes_d2h = 0;     // what upload copied up and download copied down (desc_*_batch_bytes): counters, no behaviour

    ~BatchDevice() { close(); }

    // Everything a handle holds on the device, in the one order that is safe: the stream drains before its blocks go back to the cache,
    // and goes back to the pool idle.  A handle that never opened a device makes no HIP call.  Idempotent.
    void close() {
        if (stream) { (void)hipSetDevice(device); (void)hipStreamSynchronize(stream); }
        mem.release();
        for (hipEvent_t* e : {&ev0, &ev1}) if (*e) { (void)hipEventDestroy(*e); *e = nullptr; }
        if (stream) { stream_release(stream); stream = nullptr; }
    }

    // The first device call of a handle.  `what` names the batched call in the refusal of a machine without a device -- whether the
    // runtime counts zero devices or, having no driver, fails to count.
    int open(int32_t dev, const char* what) {
        device = dev;
        int ndev = desc_device_count();
        if (ndev < 0) {                           // a machine without a driver counts no devices by failing: the same refusal, the runtime's words kept
            const std::string msg = desc_last_error();
            return fail(ndev, "no HIP device visible: %s has no CPU fallback (%s)", what, msg.c_str());
        }
        if (ndev == 0) return fail(DESC_ERR_HIP, "no HIP device visible: %s has no CPU fallback", what);
        if (dev < 0 || dev >= ndev) return fail(DESC_ERR_INVALID, "device %d out of range (0..%d)", dev, ndev - 1);
        hipError_t he = hipSetDevice(dev);
        if (he == hipSuccess) he = stream_acquire(&stream);
        if (he != hipSuccess) return fail(DESC_ERR_HIP, "device %d: %s", dev, hipGetErrorString(he));
        return DESC_OK;
    }

    // an arena block holding src[0..n) once the stream has drained; T is const where the kernel's argument record points to const
    template <class T>
    int upload(T** dst, const std::remove_const_t<T>* src, size_t n) {
        std::remove_const_t<T>* d = nullptr;
        int rc = mem.alloc(&d, n); if (rc) return rc;
        if (n) DESC_HIP(hipMemcpyAsync(d, src, sizeof(T) * n, hipMemcpyHostToDevice, stream));
        bytes_h2d += (int64_t)(sizeof(T) * n);
        *dst = d;
        return DESC_OK;
    }

    // dst[0..n) = the device array src once the stream has drained
    template <class T>
    int download(T* dst, const T* src, size_t n) {
        if (n) DESC_HIP(hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyDeviceToHost, stream));
        bytes_d2h += (int64_t)(sizeof(T) * n);
        return DESC_OK;
    }

    int timer_begin() {
        if (!ev0) DESC_HIP(hipEventCreate(&ev0));
        if (!ev1) DESC_HIP(hipEventCreate(&ev1));
        DESC_HIP(hipEventRecord(ev0, stream));
        return DESC_OK;
    }
    int timer_end() { DESC_HIP(hipEventRecord(ev1, stream)); return DESC_OK; }
    int timer_ms(float* ms) { DESC_HIP(hipEventElapsedTime(ms, ev0, ev1)); return DESC_OK; }     // after the stream has drained
};

// The body of desc_*_batch_create: argument checks, a fresh handle H, body(h); *out gets the handle only if body returned DESC_OK.
// Otherwise the handle is destroyed -- after an exception too -- and body's message is raised again, the teardown having HIP calls
// of its own.  args_ok: what the call needs besides probs.
// P: desc_problem, or the record a generator takes in its place (desc_model_spec), or the node counts of desc_align_batch_create.
template <class H, class P, class Body>
int batch_create_guarded(const char* name, H** out, const P* probs, int32_t count, Body&& body, bool args_ok = true) {
    return no_throw(name, [&]() -> int {
        if (!out) return fail(DESC_ERR_INVALID, "out is NULL");
        *out = nullptr;
        if (!args_ok || count < 0 || (count > 0 && !probs)) return fail(DESC_ERR_INVALID, "NULL argument or negative count");
        std::unique_ptr<H> h(new H());
        const int rc = body(h.get());
        if (rc) { const std::string msg = desc_last_error(); h.reset(); return fail(rc, "%s", msg.c_str()); }
        *out = h.release();
        return DESC_OK;
    });
}

}  // namespace desc
