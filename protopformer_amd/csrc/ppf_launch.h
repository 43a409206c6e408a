// The one place the library launches kernels and enqueues copies from (included at the end of ppf_common.h).
//
// One device per process: the statics below (granted dynamic LDS per kernel, the CU count) are kept per process, not per device, as the
// per-call-site flags they replace always were.  A process that drives a second GPU through this library would need them keyed by device.
#pragma once

// csrc/ppf_runtime.hip; library-internal (hidden: the exported symbols stay those of include/ppf_hip.h)
__attribute__((visibility("hidden"))) int ppf_cu_count();                      // compute units of the device, queried once (256 if the query fails)
__attribute__((visibility("hidden"))) void ppf_note_enqueue(hipStream_t s);    // the last operation on `s` is not a launch that carries a stop event

// Dynamic LDS the runtime has been asked to allow for Kernel so far (hipFuncAttributeMaxDynamicSharedMemorySize is a per-function high-water mark).
template <auto Kernel>
static int ppf_lds_granted = 0;

// Launches Kernel on `stream` with grid, block, lds_bytes and args (on an armed stream the dispatch carries the stop event
// ppf_stream_wait_stream will wait for, see ppf_common.h) and returns 0 or the hipError_t, with ppf_set_error("<who>: ...") filled in.
// The dynamic-LDS opt-in is raised only when lds_bytes exceeds what this kernel was granted before: the steady-state cost is one compare
// against a static.
template <auto Kernel, typename... Args>
static inline int ppf_launch(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const char* who, const Args&... args) {
    if ((int)lds_bytes > ppf_lds_granted<Kernel>) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) { ppf_set_error("%s: hipFuncSetAttribute: %s", who, hipGetErrorString(e)); return (int)e; }
        ppf_lds_granted<Kernel> = (int)lds_bytes;
    }
    if (hipEvent_t ev = ppf_take_stop_event(stream)) hipExtLaunchKernelGGL(Kernel, grid, block, lds_bytes, stream, nullptr, ev, 0, args...);
    else Kernel<<<grid, block, lds_bytes, stream>>>(args...);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { ppf_set_error("%s: launch failed: %s", who, hipGetErrorString(e)); return (int)e; }
    return 0;
}

// Anything else the library puts on a stream goes through these, so that an armed ppf_stream_wait_stream never waits on the stop event
// of a kernel that is no longer the stream's last operation.
static inline hipError_t ppf_memset_async(void* dst, int value, size_t bytes, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(dst, value, bytes, stream);
    ppf_note_enqueue(stream);
    return e;
}
static inline hipError_t ppf_memcpy_async(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, stream);
    ppf_note_enqueue(stream);
    return e;
}
static inline hipError_t ppf_memcpy2d_async(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height,
                                            hipMemcpyKind kind, hipStream_t stream) {
    hipError_t e = hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, kind, stream);
    ppf_note_enqueue(stream);
    return e;
}
