/*
 * qr_dev_mem.hpp - host side of the device layer: the error macros and the owners of device and page-locked memory.
 * Included by qr_device.hip only.
 *
 * No owner frees in a destructor: most of them sit in thread_local or static storage, and the HIP runtime may already be
 * shut down when those are destroyed at exit.  They release through release() alone, with the owning device made current by
 * the caller, and leak at process exit.
 */
#define HIP_TRY(expr)                                                          \
    do {                                                                       \
        hipError_t e_ = (expr);                                                \
        if (e_ != hipSuccess)                                                  \
            return qr_fail(QR_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

/* ... and for a check of our own: its refusal is the caller's */
#define QR_TRY(expr)                                                           \
    do {                                                                       \
        const int rc_ = (expr);                                                \
        if (rc_ != QR_OK) return rc_;                                          \
    } while (0)

/* Grow-only buffer.  HOST < 0: device memory, and the device is synchronised before a buffer that queued work may still use
 * is freed; otherwise page-locked host memory with these hipHostMalloc flags. */
template <int HOST>
struct GrowBuf
{
    void *p = nullptr; size_t cap = 0;
    /* room for `need` bytes, `slack` more when it has to allocate; *grew: the old buffer and its contents are gone */
    hipError_t ensure(size_t need, size_t slack = 0, bool *grew = nullptr)
    {
        if (cap >= need) return hipSuccess;
        if (grew) *grew = true;
        if (HOST < 0 && p) { const hipError_t e = hipDeviceSynchronize(); if (e != hipSuccess) return e; }
        release();
        const hipError_t e = HOST < 0 ? hipMalloc(&p, need + slack) : hipHostMalloc(&p, need + slack, (unsigned)HOST);
        if (e == hipSuccess) cap = need + slack; else p = nullptr;
        return e;
    }
    void release() { if (p) (void)(HOST < 0 ? hipFree(p) : hipHostFree(p)); p = nullptr; cap = 0; }
    template <class T> T *as() const { return (T *)p; }
};
using DevBuf   = GrowBuf<-1>;
using PinBuf   = GrowBuf<(int)hipHostMallocPortable>;      /* every device copies from / into it */
using StageBuf = GrowBuf<(int)hipHostMallocDefault>;

/* slack of a buffer that holds a scene image: an animation's image grows a little from frame to frame */
static size_t image_slack(size_t need) { return need / 2 + ((size_t)1 << 20); }

/* The counter block of a launch: QR_COUNTER_HEAD words (ray counts, QR_STATS slots 4..62), and per wave of the schedule
 * QR_WT_SLOTS more in QR_WAVETIME builds. */
#define QR_COUNTER_HEAD 64
static size_t counter_bytes(size_t n_sched)
{
#ifdef QR_WAVETIME
    return (QR_COUNTER_HEAD + QR_WT_SLOTS * n_sched) * sizeof(unsigned long long);
#else
    (void)n_sched;
    return QR_COUNTER_HEAD * sizeof(unsigned long long);
#endif
}

/* a cached counter block for a schedule of n_sched waves: zeroed when it is (re)allocated */
static hipError_t counters_ensure(DevBuf &b, size_t n_sched)
{
    bool grew = false;
    hipError_t e = b.ensure(counter_bytes(n_sched), 0, &grew);
    if (e == hipSuccess && grew && (e = hipMemset(b.p, 0, b.cap)) != hipSuccess) b.release();
    return e;
}

/* An uploaded subset of a schedule: n entries of `words_per_entry` words (2; 4 in a multi-target launch). */
struct SchedBuf
{
    uint32_t *d = nullptr; int32_t n = 0;
    hipError_t upload(const std::vector<uint32_t> &words, size_t words_per_entry)
    {
        n = (int32_t)(words.size() / words_per_entry);
        if (n == 0) return hipSuccess;
        hipError_t e = hipMalloc((void **)&d, words.size() * 4);
        if (e == hipSuccess) e = hipMemcpy(d, words.data(), words.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) release();
        return e;
    }
    void release() { (void)hipFree(d); d = nullptr; n = 0; }
};
