// devbuf.h -- the two owning types behind every device and pinned-host allocation of the engine (included from hdm_common.h).
// Move-only; empty by default; freed by the destructor, by reset() and when regrown.  hipFree synchronises the device, so a
// buffer's scope is also the point of the call sequence at which that happens: temporaries are locals, grown buffers regrow
// through reserve(), everything else goes with its owner.  Kernel argument structs take get(): an owning type never crosses
// a launch.  Nothing with static or thread-local storage duration may be one of these (hipFree after the runtime has shut
// down hangs or crashes at exit).
#pragma once

template <typename T> class HdmBuf {
    T *p = nullptr;
    size_t n = 0;
public:
    HdmBuf() = default;
    HdmBuf(const HdmBuf &) = delete;
    HdmBuf &operator=(const HdmBuf &) = delete;
    HdmBuf(HdmBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    HdmBuf &operator=(HdmBuf &&o) noexcept {
        if (this != &o) { reset(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~HdmBuf() { reset(); }
    void reset() {
        if (p) (void) hipFree(p);
        p = nullptr;
        n = 0;
    }
    // `count` elements plus `extra_bytes` of slack (hdm_operand_pad); what was held is freed first.  Through hdm_malloc, so
    // that HDM_POISON reaches it.
    hipError_t alloc(size_t count, size_t extra_bytes = 0) {
        reset();
        const hipError_t e = hdm_malloc((void **) &p, sizeof(T) * count + extra_bytes);
        if (e != hipSuccess) p = nullptr;
        else n = count;
        return e;
    }
    // no-op when `count` elements are held already; otherwise free + alloc (the contents are not kept)
    hipError_t reserve(size_t count) { return (p && n >= count) ? hipSuccess : alloc(count); }
    T *get() const { return p; }
    size_t count() const { return n; }
    explicit operator bool() const { return p != nullptr; }
};

// the same for hipHostMalloc memory; with hipHostMallocMapped the device's address of the block is kept beside the host's
template <typename T> class HdmPinned {
    T *p = nullptr, *d = nullptr;
    size_t n = 0;
public:
    HdmPinned() = default;
    HdmPinned(const HdmPinned &) = delete;
    HdmPinned &operator=(const HdmPinned &) = delete;
    HdmPinned(HdmPinned &&o) noexcept : p(o.p), d(o.d), n(o.n) { o.p = o.d = nullptr; o.n = 0; }
    HdmPinned &operator=(HdmPinned &&o) noexcept {
        if (this != &o) { reset(); p = o.p; d = o.d; n = o.n; o.p = o.d = nullptr; o.n = 0; }
        return *this;
    }
    ~HdmPinned() { reset(); }
    void reset() {
        if (p) (void) hipHostFree(p);
        p = d = nullptr;
        n = 0;
    }
    hipError_t alloc(size_t count, unsigned flags = hipHostMallocDefault) {
        reset();
        hipError_t e = hipHostMalloc((void **) &p, sizeof(T) * count, flags);
        if (e != hipSuccess) { p = nullptr; return e; }
        n = count;
        if (flags & hipHostMallocMapped) {
            e = hipHostGetDevicePointer((void **) &d, p, 0);
            if (e != hipSuccess) reset();
        }
        return e;
    }
    T *get() const { return p; }
    T *dev() const { return d; }   // mapped blocks only
    size_t count() const { return n; }
    explicit operator bool() const { return p != nullptr; }
};
