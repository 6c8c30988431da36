// host_call.hip -- the process-wide services every other unit's host code calls (declared in nmrfit_internal.h; the
// types built on them are host_call.h's): the thread-local error text, the stream cache, staged copies to pageable host
// memory, the device table and the device check -- and the entry points that take no object.  No exception leaves this file.
#include "host_call.h"
#include "nmrfit_amd_diag.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <utility>

namespace nmrfit {

static thread_local std::string g_last_error;

void set_error(const std::string &msg) { g_last_error = msg; }

int hip_fail(hipError_t e, const char *what, const char *file, int line)
{
    char buf[512];
    snprintf(buf, sizeof buf, "HIP error %d (%s) in `%s` at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
    g_last_error = buf;
    return NMRFIT_E_HIP;
}

// (the knob is read once per process; unset: one predictable branch.  The fill is the runtime's memset on the null stream and
// a wait of its own: the library's streams are non-blocking, so nothing else orders it before the caller's first use)
hipError_t device_alloc(void **p, size_t bytes)
{
    static const int poison = parse_poison_byte(getenv("NMRFIT_POISON_ALLOC"));
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess || poison < 0) return e;
    if ((e = hipMemset(*p, poison, bytes)) == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        (void)hipFree(*p);
        *p = nullptr;
    }
    return e;
}

// A context's own stream, recycled: a new HIP stream costs about 4 ms on this stack when it is first used (the hardware
// queue behind it is made then; measured, tools/archive/hip_call_costs.hip) and a whole default fit is 25 ms -- a fit
// that pyswarm's rule stops after a few hundred generations 3 ms.  Contexts that come and go (one per fitted spectrum)
// hand their idle stream to the next one on the same device instead.  NMRFIT_NO_STREAM_CACHE=1 turns it off.
namespace {
struct StreamPool {
    std::mutex lock;
    std::vector<std::pair<int, hipStream_t>> idle;
};
StreamPool &stream_pool()
{
    static StreamPool *pool = new StreamPool;   // (never destroyed: no order-of-destruction trouble at process exit)
    return *pool;
}
constexpr size_t kMaxIdleStreams = 16;
bool stream_cache_on()
{
    static const bool on = getenv("NMRFIT_NO_STREAM_CACHE") == nullptr;
    return on;
}
}  // namespace

hipError_t take_stream(int device, hipStream_t *out)
{
    if (stream_cache_on()) {
        StreamPool &pool = stream_pool();
        std::lock_guard<std::mutex> guard(pool.lock);
        for (size_t i = 0; i < pool.idle.size(); ++i)
            if (pool.idle[i].first == device) {
                *out = pool.idle[i].second;
                pool.idle.erase(pool.idle.begin() + (long)i);
                return hipSuccess;
            }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}

// (the caller has synchronised the stream: nothing is queued on it)
void give_stream(int device, hipStream_t s)
{
    if (stream_cache_on()) {
        StreamPool &pool = stream_pool();
        std::lock_guard<std::mutex> guard(pool.lock);
        if (pool.idle.size() < kMaxIdleStreams) {
            pool.idle.emplace_back(device, s);
            return;
        }
    }
    (void)hipStreamDestroy(s);
}

// Large results to PAGEABLE host memory (numpy arrays the caller has just made): a plain hipMemcpy pins the destination's
// pages on the fly, 13-26 ms for the 30 MB a batch of 50 reconstructed fits returns, 1 ms when the runtime happens to
// know the pages (tools/generate_breakdown.py; profiles/r06/generate_breakdown.txt).  Here the copy goes through two
// pinned buffers the process keeps per device: the DMA engine fills one while the CPU copies the other out, so the call
// costs what the CPU copy into the caller's pages costs (~3 ms for 30 MB) whatever the runtime's pinning cache holds.
// Synchronous: the data is in `dst` on return.  Small copies take the plain path.
namespace {
struct HostStage {
    std::mutex lock;                 // one staged copy at a time per device (the buffers are the resource)
    void *buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
};
constexpr size_t kStageChunk = (size_t)4 << 20;
constexpr size_t kStageMin = (size_t)256 << 10;
HostStage *host_stage(int device)
{
    static std::mutex table_lock;
    static std::vector<HostStage *> table;   // (never destroyed: pinned memory outlives every context, freed at process exit)
    std::lock_guard<std::mutex> guard(table_lock);
    if ((int)table.size() <= device) table.resize((size_t)device + 1, nullptr);
    if (!table[(size_t)device]) table[(size_t)device] = new HostStage;
    return table[(size_t)device];
}
}  // namespace

int staged_d2h(int device, hipStream_t st, void *dst_host, const void *src_dev, size_t bytes)
{
    if (bytes == 0) return NMRFIT_OK;
    static const bool off = getenv("NMRFIT_NO_STAGED_COPIES") != nullptr;   // A/B knob
    if (bytes < kStageMin || off) {
        NMRFIT_HIP(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, st));
        NMRFIT_HIP(hipStreamSynchronize(st));
        return NMRFIT_OK;
    }
    HostStage *hs = host_stage(device);
    std::lock_guard<std::mutex> guard(hs->lock);
    for (int i = 0; i < 2; ++i) {   // (each on its own: a call that failed between the two leaves the event to the next one)
        if (!hs->buf[i]) NMRFIT_HIP(hipHostMalloc(&hs->buf[i], kStageChunk, hipHostMallocDefault));
        if (!hs->ev[i]) NMRFIT_HIP(hipEventCreateWithFlags(&hs->ev[i], hipEventDisableTiming));
    }
    const unsigned char *src = static_cast<const unsigned char *>(src_dev);
    unsigned char *dst = static_cast<unsigned char *>(dst_host);
    const size_t n_chunks = (bytes + kStageChunk - 1) / kStageChunk;
    for (size_t i = 0; i <= n_chunks; ++i) {
        if (i < n_chunks) {   // (buffer i % 2 was copied out two rounds ago, before chunk i - 1 was waited for)
            const size_t off_i = i * kStageChunk, n = std::min(kStageChunk, bytes - off_i);
            NMRFIT_HIP(hipMemcpyAsync(hs->buf[i & 1], src + off_i, n, hipMemcpyDeviceToHost, st));
            NMRFIT_HIP(hipEventRecord(hs->ev[i & 1], st));
        }
        if (i > 0) {
            const size_t off_p = (i - 1) * kStageChunk, n = std::min(kStageChunk, bytes - off_p);
            NMRFIT_HIP(hipEventSynchronize(hs->ev[(i - 1) & 1]));
            memcpy(dst + off_p, hs->buf[(i - 1) & 1], n);
        }
    }
    return NMRFIT_OK;
}

// (hipGetDeviceProperties costs about a millisecond: once per device and PROCESS -- a default fit is 30 ms, and
// fit_many's worker threads come and go)
int device_info_cached(int device, DeviceInfo *out)
{
    static std::mutex dev_lock;
    static std::vector<DeviceInfo> dev_cache;
    std::lock_guard<std::mutex> guard(dev_lock);
    if ((int)dev_cache.size() <= device) dev_cache.resize((size_t)device + 1);
    if (!dev_cache[(size_t)device].known) {
        hipDeviceProp_t hp;
        NMRFIT_HIP(hipGetDeviceProperties(&hp, device));
        dev_cache[(size_t)device].cus = hp.multiProcessorCount;
        strncpy(dev_cache[(size_t)device].arch, hp.gcnArchName, sizeof(dev_cache[0].arch) - 1);
        dev_cache[(size_t)device].known = true;
    }
    *out = dev_cache[(size_t)device];
    return NMRFIT_OK;
}

// the index names one of the visible devices; `to_work_on`: a call that needs a device says so when there is none at all
static int check_device_index(int device, bool to_work_on)
{
    int n = 0;
    const int rc = nmrfit_device_count(&n);
    if (rc != NMRFIT_OK) return rc;
    if (n == 0 && to_work_on) return refuse(NMRFIT_E_NO_DEVICE, "no HIP device visible: libnmrfit_amd has no CPU fallback");
    if (device < 0 || device >= n) return refuse(NMRFIT_E_NO_DEVICE, "device index out of range");
    return NMRFIT_OK;
}

int use_device(int device, DeviceInfo *info)
{
    int rc = check_device_index(device, true);
    if (rc != NMRFIT_OK) return rc;
    NMRFIT_HIP(hipSetDevice(device));
    DeviceInfo prop;
    if ((rc = device_info_cached(device, &prop)) != NMRFIT_OK) return rc;
    if (strncmp(prop.arch, "gfx950", 6) != 0) {
        set_error(std::string("device is ") + prop.arch + ", this library is built for gfx950 only");
        return NMRFIT_E_NO_DEVICE;
    }
    if (info) *info = prop;
    return NMRFIT_OK;
}

int check_spectra_count(const char *who, int32_t S)
{
    if (S < 1 || S > 65535) {
        set_error(std::string(who) + ": S must be 1..65535");
        return NMRFIT_E_INVALID;
    }
    return NMRFIT_OK;
}

}  // namespace nmrfit

using namespace nmrfit;

#pragma GCC visibility push(default)   // the C-ABI: the only symbols the library exports (build.sh: -fvisibility=hidden)
extern "C" {

int nmrfit_abi_version(void) { return NMRFIT_ABI_VERSION; }

int nmrfit_diag_ab_build(void)
{
#ifdef NMRFIT_AB_BUILD
    return 1;
#else
    return 0;
#endif
}

const char *nmrfit_last_error(void) { return g_last_error.c_str(); }

int nmrfit_device_count(int *count)
{
    if (!count) {
        set_error("null count pointer");
        return NMRFIT_E_INVALID;
    }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        (void)hipGetLastError();
        set_error(std::string("hipGetDeviceCount failed: ") + hipGetErrorString(e));
        return NMRFIT_E_NO_DEVICE;
    }
    *count = n;
    return NMRFIT_OK;
}

int nmrfit_device_info(int device, char *name, int name_len, int *compute_units, char *arch, int arch_len)
{
    const int rc = check_device_index(device, false);
    if (rc != NMRFIT_OK) return rc;
    hipDeviceProp_t prop;
    NMRFIT_HIP(hipGetDeviceProperties(&prop, device));
    if (name && name_len > 0) {
        strncpy(name, prop.name, (size_t)name_len - 1);
        name[name_len - 1] = 0;
    }
    if (arch && arch_len > 0) {
        strncpy(arch, prop.gcnArchName, (size_t)arch_len - 1);
        arch[arch_len - 1] = 0;
    }
    if (compute_units) *compute_units = prop.multiProcessorCount;
    return NMRFIT_OK;
}

int nmrfit_device_pci_bus_id(int device, char *buf, int len)
{
    const int rc = check_device_index(device, false);
    if (rc != NMRFIT_OK) return rc;
    if (!buf || len < 16) {
        set_error("nmrfit_device_pci_bus_id: buffer of at least 16 bytes");
        return NMRFIT_E_INVALID;
    }
    NMRFIT_HIP(hipDeviceGetPCIBusId(buf, len, device));
    return NMRFIT_OK;
}

}  // extern "C"
#pragma GCC visibility pop
