// api.hip -- library-level entry points: version, thread-local error text, tuning options, HIP-event stopwatch.
#include "common.h"
#include <atomic>
#include <cstring>
#include <mutex>
#include <algorithm>
#include <unordered_map>
#include <map>
#include <string>
#include <vector>

namespace mi355 {
static thread_local char g_err[512] = "";

// ---- tuning options: ONE BLOCK PER DEVICE --------------------------------------------------------------------------------------
// mi355_set_option / mi355_get_option act on the block of the calling thread's CURRENT device (hipGetDevice), and every launch reads
// the block of the device it launches on: a host that drives eight GPUs from one process (one thread per GPU) can tune --
// or, in a test, sabotage -- one device without the others seeing it.  A block starts from the defaults in options.h.
constexpr int MAX_DEV = 64;
struct OptDesc { const char* key; long def, lo, hi; };
static const OptDesc kOpts[O_COUNT] = {             // from the same list as enum Opt (common.h), so row i describes option i
#define MI355_OPT(id, key, def, lo, hi) {key, def, lo, hi},
#include "options.h"
#undef MI355_OPT
};
namespace {
constexpr long OPT_UNSET = (long)0x8000000000000000ull;              // a device block entry that follows the process default
struct OptBlock { std::atomic<long> v[O_COUNT]; };
OptBlock g_opt[MAX_DEV];                 // per-device overrides (mi355_set_option on the current device)
std::atomic<long> g_def[O_COUNT];        // process defaults (mi355_set_default_option): what a device without an override reads
std::once_flag g_opt_once;
int cur_dev() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    return dev >= 0 && dev < MAX_DEV ? dev : 0;
}
void init_opts() {
    std::call_once(g_opt_once, [] {
        for (int i = 0; i < O_COUNT; ++i) g_def[i].store(kOpts[i].def, std::memory_order_relaxed);
        for (auto& b : g_opt)
            for (int i = 0; i < O_COUNT; ++i) b.v[i].store(OPT_UNSET, std::memory_order_relaxed);
    });
}
}  // namespace
long opt(Opt o) {
    init_opts();
    const long v = g_opt[cur_dev()].v[o].load(std::memory_order_relaxed);
    return v != OPT_UNSET ? v : g_def[o].load(std::memory_order_relaxed);
}

char* err_buf() { return g_err; }

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// ---- workspaces of the granule-exchange kernels (chan_fused.hip, cbam_single.hip, chan_stat.hip) ---------------------------------
// A granule is valid when it carries the tag of the CURRENT launch = the workspace's epoch word + 1 (advanced on the device by the
// launch's last ticket draw), so a slot written by any earlier launch can never look valid and the region only has to be zeroed
// when its history is unknown: first use of the pointer, a different layout key, or "ws_persistent" off (the default: a C caller
// that frees / reuses workspace memory between calls must not opt in).  Nothing about a launch lives on the host, which is what
// lets these kernels be recorded by hipGraph capture.
namespace {
struct WsEntry { unsigned long long key; };
std::mutex g_ws_mu;
std::unordered_map<const void*, WsEntry> g_ws;
}  // namespace

bool stream_is_capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return cs != hipStreamCaptureStatusNone;
}

// Workspaces of the kernels that keep their launch tag in device memory (se_single_kernel, cbam_single_kernel): the host only has to know whether the
// region was zeroed for this shape.  Under stream capture an unknown region stays unknown (the memset the caller records runs at
// replay time, not now); a known one needs nothing.
static bool ws_known(const void* region, unsigned long long key, hipStream_t st) {
    if (!opt(O_WS_PERSISTENT)) return false;
    std::lock_guard<std::mutex> lk(g_ws_mu);
    auto it = g_ws.find(region);
    if (it != g_ws.end() && it->second.key == key) return true;
    if (!stream_is_capturing(st)) g_ws[region] = WsEntry{key};
    return false;
}
// Zero an exchange area with a KERNEL.  Under stream capture a recorded hipMemsetAsync did not reliably take effect before the kernel
// node behind it on this runtime (ROCm 7.2: the second of two back-to-back memset nodes -- a replayed SE launch saw the granules of
// the previous replay); a kernel node is ordered like any other launch, so the exchange kernels zero their areas this way everywhere.
namespace {
__global__ __launch_bounds__(256) void ws_zero_kernel(unsigned* p, size_t words) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) p[i] = 0u;
}
}  // namespace
static hipError_t ws_zero_async(void* p, size_t bytes, hipStream_t st) {
    const size_t words = bytes / 4;                                    // callers pass multiples of 4 bytes, 4-byte aligned
    if (!words) return hipSuccess;
    size_t blocks = (words + 1023) / 1024;
    if (blocks > 2048) blocks = 2048;
    ws_zero_kernel<<<(int)blocks, 256, 0, st>>>(static_cast<unsigned*>(p), words);
    return hipGetLastError();
}
void ws_forget(const void* region) {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    g_ws.erase(region);
}
void ws_forget_range(const void* base, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    const char* lo = static_cast<const char*>(base);
    for (auto it = g_ws.begin(); it != g_ws.end();) {
        const char* p = static_cast<const char*>(it->first);
        if (p >= lo && p < lo + bytes) it = g_ws.erase(it);
        else ++it;
    }
}

// ---- exchange-kernel failure word + fp16 range word (common.h): ONE PAIR PER CALLING THREAD AND DEVICE -------------------------
// One pinned, device-visible allocation, made once (never inside a stream capture): THREAD_SLOTS + 1 slots of 64 bytes per device
// ordinal; in a device's 64 bytes, word 0 = exchange failure code, word 4 = range code.  A launch hands its kernel the words of the
// thread that issues it, on the device it runs on, and the host checks the calling thread's words on its current device: one thread's
// time-out or fp16 overflow never fails another thread's next call, and one thread's mi355_range_wait never absorbs (clears) another
// thread's report -- a serving process that runs one module per thread on one GPU.  A thread takes a free slot on first use and hands it
// back when it exits; a slot is cleared when it is handed out again.  Threads beyond THREAD_SLOTS alive at once share the last
// (overflow) slot and see each other's reports, as every thread of a device did before.  A hipGraph captured on thread T holds T's words
// in its kernel nodes: its replays report into T's slot, whichever thread replays it -- check from T (or after T has exited, from
// whichever thread holds the slot then).
namespace {
constexpr int THREAD_SLOTS = 64;
constexpr size_t SLOT_WORDS = 16 * MAX_DEV;
std::once_flag g_sync_once;
unsigned* g_sync_block = nullptr;
std::mutex g_slot_mu;
bool g_slot_used[THREAD_SLOTS] = {};
struct ThreadSlot {
    int idx = -1;                                      // THREAD_SLOTS = the shared overflow slot
    ~ThreadSlot() {
        if (idx < 0 || idx >= THREAD_SLOTS) return;
        std::lock_guard<std::mutex> lk(g_slot_mu);
        g_slot_used[idx] = false;
    }
};
thread_local ThreadSlot t_slot;
// the calling thread's words on its current device; null while the block does not exist (or its allocation failed)
unsigned* thread_words() {
    if (!g_sync_block) return nullptr;
    if (t_slot.idx < 0) {
        std::lock_guard<std::mutex> lk(g_slot_mu);
        int i = 0;
        while (i < THREAD_SLOTS && g_slot_used[i]) ++i;
        if (i < THREAD_SLOTS) {
            g_slot_used[i] = true;
            std::memset(g_sync_block + i * SLOT_WORDS, 0, SLOT_WORDS * sizeof(unsigned));   // a previous owner's codes are not ours
        }
        t_slot.idx = i;
    }
    return g_sync_block + t_slot.idx * SLOT_WORDS + 16 * cur_dev();
}
}  // namespace
unsigned* sync_err_word() {
    std::call_once(g_sync_once, [] {
        const size_t bytes = (THREAD_SLOTS + 1) * SLOT_WORDS * sizeof(unsigned);
        void* p = nullptr;
        if (hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable) == hipSuccess && p) {
            std::memset(p, 0, bytes);
            g_sync_block = static_cast<unsigned*>(p);
        } else {
            (void)hipGetLastError();
        }
    });
    return thread_words();
}
// sync_err_word(), but never allocates inside a stream capture (may return null there)
static unsigned* sync_err_word_on(hipStream_t st) {
    if (!g_sync_block && stream_is_capturing(st)) return nullptr;         // never allocate pinned memory inside a capture
    return sync_err_word();
}
// ---- "which launch do I have to wait for before the range word is final?" (round 6: mi355_range_arm / mi355_range_wait) ---------------
// While a thread has armed its current device, every launcher that hands a kernel the range word (range_word() below: the fp16 producers)
// counts itself and marks the device dirty.  mi355_range_wait() must synchronise on an event that lies BEHIND the last producer; recording one behind every
// producer would put ~50 marker packets into a ViT-Base forward (measured: +0.13 ms of 12.1), so the caller PREDICTS the last producer --
// mi355_range_arm(1 + k): "the k-th producer since this call is the last one", the count its previous forward of the same module reported
// (mi355_range_launches) -- and the ONE event of the forward is recorded in front of the first launch that follows the k-th producer
// (TraceScope's constructor sits in front of every instrumented launch).  The non-reporting launches queued behind it (attention core,
// fp32-output projections, fc2) then keep the GPU busy while the host already returns.  A wrong or missing prediction costs slack, never
// correctness: a producer launched after the event marks the device dirty again and mi355_range_wait() records a second event at the tail.
// The marks are per calling thread and device (like the words above): arm, count, event and stream of one thread never see another's
// launches.  At thread exit the events go back to a per-device pool that later threads draw from (no HIP call at thread exit, which may
// come after the runtime has shut down); the pool never holds more events than threads have been alive at once.
namespace {
struct RangeMark {
    int armed = 0, dirty = 0, fresh = 0, have = 0, count = 0, expect = 0;
    hipEvent_t ev = nullptr;
    hipStream_t st = nullptr;
};
std::mutex g_ev_mu;
std::vector<hipEvent_t> g_ev_pool[MAX_DEV];
struct ThreadMarks {
    RangeMark m[MAX_DEV];
    ~ThreadMarks() {
        std::lock_guard<std::mutex> lk(g_ev_mu);
        for (int d = 0; d < MAX_DEV; ++d)
            if (m[d].ev) g_ev_pool[d].push_back(m[d].ev);
    }
};
thread_local ThreadMarks t_marks;
RangeMark& rmark(int dev) { return t_marks.m[dev]; }
void range_mark_record(RangeMark& m, int dev) {
    m.dirty = 0;
    if (stream_is_capturing(m.st)) return;                                // never record the thread's event into a graph
    if (!m.ev) {
        {
            std::lock_guard<std::mutex> lk(g_ev_mu);
            if (!g_ev_pool[dev].empty()) { m.ev = g_ev_pool[dev].back(); g_ev_pool[dev].pop_back(); }
        }
        if (!m.ev && hipEventCreateWithFlags(&m.ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); m.ev = nullptr; return; }
    }
    if (hipEventRecord(m.ev, m.st) == hipSuccess) m.have = 1;
    else (void)hipGetLastError();
}
}  // namespace
// A producer ENTRY may issue several launches (split rounds, helper passes): range_word() only opens it (pending), the entry's closing
// MI355_LAUNCH_CHECK marks the device dirty, and no event is ever recorded while an entry is open -- so the event always lies behind every
// launch of the producer it covers.
void range_mark_before_launch() {                                          // TraceScope: in front of every instrumented launch
    const int dev = cur_dev();
    RangeMark& m = rmark(dev);
    if (!m.dirty || m.fresh) return;
    if (m.expect > 0 && m.count >= m.expect) range_mark_record(m, dev);
}
void range_mark_entry_done() {                                             // MI355_LAUNCH_CHECK: the launches of the current entry are all enqueued
    RangeMark& m = rmark(cur_dev());
    if (!m.fresh) return;
    m.fresh = 0;
    m.dirty = 1;
}
unsigned* range_word(hipStream_t st) {
    if (!g_sync_block && stream_is_capturing(st)) return nullptr;         // never allocate pinned memory inside a capture
    unsigned* w = sync_err_word();
    if (w) {
        RangeMark& m = rmark(cur_dev());
        if (m.armed) {
            m.st = st;
            ++m.count;
            m.fresh = 1;                                                   // an open producer entry ("pending")
        }
    }
    return w ? w + 4 : nullptr;                                            // second quarter of the thread's 64 bytes of the device
}
int range_arm(int on) {
    RangeMark& m = rmark(cur_dev());
    m.dirty = 0;
    m.fresh = 0;
    m.have = 0;
    if (on) m.count = 0;                                                   // a disarm keeps the count for mi355_range_launches()
    m.expect = on > 1 ? on - 1 : 0;
    m.armed = on ? 1 : 0;
    return MI355_OK;
}
long range_launches() { return rmark(cur_dev()).count; }
int range_wait() {
    const int dev = cur_dev();
    RangeMark& m = rmark(dev);
    if (m.fresh) { m.fresh = 0; m.dirty = 1; }
    if (m.dirty) range_mark_record(m, dev);                                // no event behind the last producer yet: at the tail of the stream
    if (m.have && m.ev) {
        if (hipEventSynchronize(m.ev) != hipSuccess) return fail(MI355_EHIP, "mi355_range_wait: hipEventSynchronize -> %s", hipGetErrorString(hipGetLastError()));
        m.have = 0;
    }
    return range_pending("mi355_range_wait");
}
int range_pending(const char* who) {
    unsigned* w = thread_words();
    if (w) w += 4;
    if (!w || !__atomic_load_n(w, __ATOMIC_ACQUIRE)) return MI355_OK;
    const unsigned code = __atomic_exchange_n(w, 0u, __ATOMIC_ACQ_REL);
    if (!code) return MI355_OK;
    static const char* const names[] = {"?", "mi355_cast16_fwd", "mi355_layernorm16_fwd", "a 16-bit-output GEMM epilogue (mi355_linear16_fwd family) or the 16-bit store of mi355_proj_mlp_fused_x16_fwd / mi355_mlp_fused_o16_fwd",
                                        "a fused block kernel (mi355_mlp_fused_fwd / mi355_proj_mlp_fused_fwd / mi355_cswin_stripe_attn_fwd / "
                                        "mi355_ln_linear16_fwd / mi355_layernorm16_t_fwd / mi355_mixer_token_fwd)",
                                        "the LayerNorm-folding GEMM epilogue (mi355_linear16_lnc_fwd / mi355_ln_center16_fwd)",
                                        "the fp16 operand staging of an fp32-input GEMM (mi355_linear_fwd / mi355_token_mix_fwd / mi355_conv2d_tokens_fwd / "
                                        "mi355_patch_embed_fwd / mi355_patch_embed_ws_fwd)",
                                        "the fp16 q / k / v staging of an fp32-I/O attention core (mi355_sdpa_fwd / mi355_sdpa_general_fwd / "
                                        "mi355_cswin_lepe_attn_fwd)",
                                        "a DoubleAttention kernel (mi355_double_attn_fwd: x, the A product, G, M' or the weights staged to fp16)"};
    return fail(MI355_ERANGE, "%s: an EARLIER launch of %s converted a finite value of magnitude >= 65520 to fp16: that tensor holds inf "
                "where the fp32 reference is finite.  Run the module in precision 0 (strict) or 2 (bf16)", who, names[code < 9 ? code : 0]);
}
unsigned spin_limit() { return (unsigned)opt(O_SPIN_LIMIT); }
int sync_pending(const char* who) {
    unsigned* w = sync_err_word();
    if (!w) return MI355_OK;
    if (!__atomic_load_n(w, __ATOMIC_ACQUIRE)) return MI355_OK;
    const unsigned code = __atomic_exchange_n(w, 0u, __ATOMIC_ACQ_REL);       // read AND clear: a code stored in between is not lost
    if (!code) return MI355_OK;
    static const char* const names[] = {"?", "SE (se_single_kernel)", "CBAM (cbam_single_kernel)", "channel-statistics gate (stat_single_kernel)",
                                        "the persistent GEMM's split last round (gemm16_p8_kernel)"};
    return fail(MI355_ESYNC, "%s: an inter-workgroup exchange of an EARLIER launch of %s ran out of its poll budget (%u sweeps): that launch's "
                "output is invalid.  Typical cause: fewer workgroups resident than one image needs (partitioned / masked device)",
                who, names[code < 5 ? code : 0], spin_limit());
}
// ---- host half of the granule-exchange protocol (common.h): the one place where a failed zeroing or launch forgets the region ----
int xch_begin(const char* who, hipStream_t st, unsigned** herr, unsigned* spin) {
    *herr = sync_err_word_on(st);
    *spin = spin_limit();
    return sync_pending(who);
}
int xch_zero(const char* who, void* region, unsigned long long key, size_t bytes, hipStream_t st) {
    if (ws_known(region, key, st)) return MI355_OK;      // unknown history: first use, another layout key, "ws_persistent" off
    const hipError_t e = ws_zero_async(region, bytes, st);
    if (e == hipSuccess) return MI355_OK;
    ws_forget(region);
    return fail(MI355_EHIP, "%s: zeroing -> %s", who, hipGetErrorString(e));
}
int xch_launched(const char* who, const void* region) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return MI355_OK;
    if (region) ws_forget(region);
    return fail(MI355_EHIP, "%s: launch -> %s", who, hipGetErrorString(e));
}
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the CURRENT device and is a LIMIT: remember the largest byte count set per
// (kernel, device ordinal) and raise it when a later launch asks for more (a kernel whose dynamic LDS depends on the shape --
// double_attn_small: HW * 64 + 43008 -- first run on a small image would otherwise fail on a larger one).
int func_dynamic_lds(const void* fn, int bytes) {
    static std::mutex mu;
    static std::unordered_map<const void*, std::unordered_map<int, int>> done;      // kernel -> device ordinal -> bytes configured
    const int dev = cur_dev();
    std::lock_guard<std::mutex> lk(mu);
    int& have = done[fn][dev];
    if (have >= bytes) return MI355_OK;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return fail(MI355_EHIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize, %d) -> %s", bytes, hipGetErrorString(e));
    have = bytes;
    return MI355_OK;
}
// ---- in-process kernel tally (common.h TraceScope) --------------------------------------------------------------------------------
namespace {
struct TraceRec { std::string tag; hipEvent_t a, b; };
std::atomic<int> g_trace_dev{-1};             // device ordinal with an open trace, -1 = none
std::mutex g_trace_mu;
std::vector<TraceRec> g_trace;
std::string g_trace_report;                   // finished report of the last closed trace, kept until it has been handed out whole
bool g_trace_report_pending = false;
}  // namespace
bool trace_on() { return g_trace_dev.load(std::memory_order_relaxed) >= 0; }
TraceScope::TraceScope(hipStream_t st_, const char* fmt, ...) : idx(-1), st(st_) {
    range_mark_before_launch();
    const int dev = g_trace_dev.load(std::memory_order_relaxed);
    if (dev < 0 || dev != cur_dev() || stream_is_capturing(st_)) return;
    char tag[160];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(tag, sizeof(tag), fmt, ap);
    va_end(ap);
    TraceRec r{tag, nullptr, nullptr};
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess || hipEventRecord(r.a, st_) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    std::lock_guard<std::mutex> lk(g_trace_mu);
    idx = (int)g_trace.size();
    g_trace.push_back(r);
}
TraceScope::~TraceScope() {
    if (idx < 0) return;
    std::lock_guard<std::mutex> lk(g_trace_mu);
    if (idx < (int)g_trace.size()) (void)hipEventRecord(g_trace[idx].b, st);
}
int trace_begin() {
    std::lock_guard<std::mutex> lk(g_trace_mu);
    for (auto& r : g_trace) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    g_trace.clear();
    g_trace_report.clear();
    g_trace_report_pending = false;
    g_trace_dev.store(cur_dev(), std::memory_order_relaxed);
    return MI355_OK;
}
// closes the trace, waits for the recorded launches and writes one line per tag: "count\ttotal_us\tmin_us\tmax_us\ttag\n", largest
// total first; returns the number of bytes the full report needs (like snprintf).  A report that did not fit (or buf == NULL) is KEPT:
// the caller sizes a buffer from the return value and calls again; it is dropped once it has been handed out whole, or by the next
// mi355_trace_begin.
long trace_end(char* buf, size_t n) {
    g_trace_dev.store(-1, std::memory_order_relaxed);
    std::lock_guard<std::mutex> lk(g_trace_mu);
    if (!g_trace.empty() || !g_trace_report_pending) {
        struct Acc { long cnt; double tot, mn, mx; };
        std::map<std::string, Acc> acc;
        for (auto& r : g_trace) {
            float ms = 0.f;
            if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
                auto it = acc.find(r.tag);
                const double us = ms * 1e3;
                if (it == acc.end()) acc[r.tag] = Acc{1, us, us, us};
                else { it->second.cnt++; it->second.tot += us; if (us < it->second.mn) it->second.mn = us; if (us > it->second.mx) it->second.mx = us; }
            } else {
                (void)hipGetLastError();
            }
            (void)hipEventDestroy(r.a);
            (void)hipEventDestroy(r.b);
        }
        g_trace.clear();
        std::vector<std::pair<std::string, Acc>> rows(acc.begin(), acc.end());
        std::sort(rows.begin(), rows.end(), [](const auto& x, const auto& y) { return x.second.tot > y.second.tot; });
        g_trace_report.clear();
        char line[256];
        for (auto& kv : rows) {
            snprintf(line, sizeof(line), "%ld\t%.1f\t%.1f\t%.1f\t%s\n", kv.second.cnt, kv.second.tot, kv.second.mn, kv.second.mx, kv.first.c_str());
            g_trace_report += line;
        }
        g_trace_report_pending = true;
    }
    const std::string& out = g_trace_report;
    const long need = (long)out.size();
    if (buf && n) {
        const size_t m = out.size() < n - 1 ? out.size() : n - 1;
        std::memcpy(buf, out.data(), m);
        buf[m] = 0;
        if (m == out.size()) {                       // handed out whole: nothing to keep
            g_trace_report.clear();
            g_trace_report_pending = false;
        }
    }
    return need;
}

int resident_slots(int per_cu) {
    int dev = 0, ncu = 256;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) { (void)hipGetLastError(); ncu = 256; }
    return ncu * per_cu;
}

static int opt_index(const char* key) {
    for (int i = 0; i < O_COUNT; ++i)
        if (std::strcmp(key, kOpts[i].key) == 0) return i;
    return -1;
}
int opt_set(const char* key, long value, bool as_default) {
    const int i = opt_index(key);
    if (i < 0) return fail(MI355_EINVAL, "mi355_set_option: unknown key '%s'", key);
    const bool ok = (value >= kOpts[i].lo && value <= kOpts[i].hi) || (i == O_SPIN_LIMIT && value == 0);
    if (!ok) return fail(MI355_EINVAL, "mi355_set_option: '%s' accepts %ld .. %ld, got %ld", key, kOpts[i].lo, kOpts[i].hi, value);
    init_opts();
    if (as_default) g_def[i].store(value, std::memory_order_relaxed);
    else g_opt[cur_dev()].v[i].store(value, std::memory_order_relaxed);
    return MI355_OK;
}
long opt_get(const char* key) {
    const int i = key ? opt_index(key) : -1;
    if (i < 0) {
        fail(MI355_EINVAL, "mi355_get_option: unknown key '%s'", key ? key : "(null)");
        return -1;
    }
    return opt((Opt)i);
}
}  // namespace mi355

struct mi355_timer {
    hipEvent_t a, b;
};

extern "C" {

int mi355_version(void) { return MI355_ABI_VERSION; }
const char* mi355_last_error(void) { return mi355::err_buf(); }

int mi355_set_option(const char* key, long value) {
    MI355_CHECK_ARG(key != nullptr);
    return mi355::opt_set(key, value, false);
}

int mi355_set_default_option(const char* key, long value) {
    MI355_CHECK_ARG(key != nullptr);
    return mi355::opt_set(key, value, true);
}

int mi355_workspace_forget(const void* ws, size_t ws_bytes) {
    MI355_CHECK_ARG(ws != nullptr);
    mi355::ws_forget_range(ws, ws_bytes);
    return MI355_OK;
}

long mi355_get_option(const char* key) { return mi355::opt_get(key); }

int mi355_trace_begin(void) { return mi355::trace_begin(); }
long mi355_trace_end(char* report, size_t report_bytes) { return mi355::trace_end(report, report_bytes); }

int mi355_sync_status(void) { return mi355::sync_pending("mi355_sync_status"); }
int mi355_range_status(void) { return mi355::range_pending("mi355_range_status"); }
// SURVEY.md 8(b) spellings (include/mi355attn.h, last section): same arguments, same code
int mi355_sdpa_core_fwd(const float* qkv, float* out, int B, int N, int heads, int d, float scale, int precision, mi355_stream_t stream) {
    return mi355_sdpa_fwd(qkv, out, B, N, heads, d, scale, precision, stream);
}
size_t mi355_sdpa_core_workspace_bytes(int, int, int, int) { return 0; }
int mi355_gemm_bias_act_fwd(const float* X, const float* W, const float* bias, const float* gamma, const float* resid, float* Y, int M, int N,
                            int K, int ldx, int ldy, int act, int precision, mi355_stream_t stream) {
    return mi355_linear_fwd(X, W, bias, gamma, resid, Y, M, N, K, ldx, ldy, act, precision, stream);
}
size_t mi355_gemm_bias_act_workspace_bytes(int, int, int) { return 0; }
int mi355_mixer_token_mlp_fwd(const float* x, const float* ln_w, const float* ln_b, float ln_eps, const void* w1p16, const float* b1,
                              const void* w2s16, const float* b2, float* y, int B, int N, int C, int T, int precision, void* ws,
                              size_t ws_bytes, mi355_stream_t stream) {
    return mi355_mixer_token_fwd(x, ln_w, ln_b, ln_eps, w1p16, b1, w2s16, b2, y, B, N, C, T, precision, ws, ws_bytes, stream);
}
size_t mi355_mixer_token_mlp_workspace_bytes(int B, int N, int C) { return mi355_mixer_token_workspace_bytes(B, N, C); }
size_t mi355_cswin_lepe_attn_workspace_bytes(int, int, int) { return 0; }
size_t mi355_xca_workspace_bytes(int, int, int, int) { return 0; }
size_t mi355_layernorm_workspace_bytes(int, int) { return 0; }
int mi355_range_arm(int on) { return mi355::range_arm(on); }
int mi355_range_wait(void) { return mi355::range_wait(); }
long mi355_range_launches(void) { return mi355::range_launches(); }

int mi355_event_time_begin(mi355_stream_t stream, void** handle) {
    MI355_CHECK_ARG(handle != nullptr);
    mi355_timer* t = new mi355_timer;
    hipError_t e = hipEventCreate(&t->a);
    if (e == hipSuccess) e = hipEventCreate(&t->b);
    if (e == hipSuccess) e = hipEventRecord(t->a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        delete t;
        return mi355::fail(MI355_EHIP, "mi355_event_time_begin: %s", hipGetErrorString(e));
    }
    *handle = t;
    return MI355_OK;
}

int mi355_event_time_end(mi355_stream_t stream, void* handle, float* ms_out) {
    MI355_CHECK_ARG(handle != nullptr && ms_out != nullptr);
    mi355_timer* t = static_cast<mi355_timer*>(handle);
    hipError_t e = hipEventRecord(t->b, static_cast<hipStream_t>(stream));
    if (e == hipSuccess) e = hipEventSynchronize(t->b);
    if (e == hipSuccess) e = hipEventElapsedTime(ms_out, t->a, t->b);
    (void)hipEventDestroy(t->a);
    (void)hipEventDestroy(t->b);
    delete t;
    if (e != hipSuccess) return mi355::fail(MI355_EHIP, "mi355_event_time_end: %s", hipGetErrorString(e));
    return MI355_OK;
}

}  // extern "C"
