// share.hpp -- several processes on one device: the per-device lock, the slot files and their count, the driver's own
// account (sysfs), the staged-or-persistent policy with its once-per-call memo.  Host only, no HIP header: the one thing
// it needs from the runtime, a device's PCI bus id, comes through share_bus_id, which the including file defines.
#pragma once
#include <errno.h>
#include <dirent.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <mutex>
#include <string>

#include "abi_error.hpp"

// the PCI bus id of a device ("0000:c1:00.0"), empty where the runtime does not say: defined by the including file
static std::string share_bus_id(int device);

// ---- several processes on one device ------------------------------------------------------------------------------
// The reference forks one worker PROCESS per chunk (psoap/sample_parallel.py:258-278); with more chunks than GPUs several
// of them share a device.  Two things then go wrong with persistent kernels:
//   * two persistent launches of different processes on the device at once starve each other (every workgroup that holds
//     a ticket is assumed to run): bounded waits time out, values come back wrong;
//   * the device suspends running workgroups (compute wave save / restore) when more than eight processes or too many
//     hardware queues share it, and resumes them on other compute units: see dag_where() in dag_kernel.hpp.
// What the library does (round 5):
//   1. an advisory per-device lock between the processes of ONE user -- flock on <dir>/gpu_<PCI bus id>.lock, <dir> =
//      $PSOAP_LOCK_DIR, else $XDG_RUNTIME_DIR/psoap, else /tmp/psoap-<uid> (0700, owner checked, never followed through a
//      symlink) -- held from an upload to the fetch of the evaluation that reads it, counted within a process, with a
//      time-out (PSOAP_DEVICE_LOCK_TIMEOUT_S, default 300) that ends in an error naming the holder instead of a hang;
//   2. a count of the cooperating processes per device (slot files beside the lock, locked for the life of the process,
//      re-counted a few times per second): share_procs();
//   3. every persistent launch reports workgroups that MOVED while they ran (DagCtl::pad[3]); a tainted evaluation is
//      run again (PSOAP_SHARE_RETRIES, default 3, same task list: bit-identical results), then evaluated by the staged
//      path (chol_kernels.hpp: kernel boundaries instead of hand-offs inside a kernel -- immune to both failures);
//   4. where the persistent kernel cannot be made safe -- several processes on the device WITHOUT the lock
//      (PSOAP_DEVICE_LOCK=0), or more of them than PSOAP_SHARE_DAG_MAX (8: the process contexts the device keeps mapped) --
//      evaluations take the staged path from the start, and take it WITHOUT the lock: kernels that synchronise at their
//      boundaries only have nothing to keep apart, and the device interleaves them (16 processes, N = 6000: 143
//      evaluations per second in all, against 91 with persistent launches taking turns under the lock -- one of 38,400 of
//      those still wrong despite the retries -- and 16 with staged evaluations taking turns: profiles/r5_share_*.txt).
//      Streams (resident launches) are refused in that regime.
// PSOAP_SHARE_POLICY=dag|staged pins the path whatever the count (experiments, tools/shared_gpu_probe.py).
struct DeviceLock {
    std::mutex mu;                    // guards the fields below (one per device: a wait on one device never blocks another)
    std::condition_variable cv;
    int fd = -1;
    int refs = 0;
    bool held = false, acquiring = false, broken = false;
    pid_t pid = 0;
    std::string path;
};
static std::mutex g_devlock_mu;        // guards the maps only
static std::map<int, DeviceLock> g_devlocks;

static bool device_lock_enabled()
{
    static const bool on = !(getenv("PSOAP_DEVICE_LOCK") && getenv("PSOAP_DEVICE_LOCK")[0] == '0');
    return on;
}
static double device_lock_timeout_s()
{
    const char* e = getenv("PSOAP_DEVICE_LOCK_TIMEOUT_S");
    return (e && atof(e) > 0.0) ? atof(e) : 300.0;
}

// process-wide counters of what sharing cost (psoap_share_stats)
struct ShareStats {
    std::atomic<long long> dag_launches{0}, tainted{0}, retries{0}, staged_fallbacks{0}, staged_policy{0}, moved_tasks{0},
        moved_xcd{0}, lock_acquisitions{0}, lock_wait_us{0}, stream_resubmits{0};
};
static ShareStats g_share;

// The per-user directory of the lock and slot files; empty when none can be had (the caller then runs unserialised and
// says so once).  Created 0700; refused when it is a symlink, not a directory, or somebody else's.
static const std::string& share_dir()
{
    static std::string dir;
    static std::once_flag once;
    std::call_once(once, [] {
        std::string d;
        if (const char* e = getenv("PSOAP_LOCK_DIR")) d = e;
        else if (const char* x = getenv("XDG_RUNTIME_DIR")) d = std::string(x) + "/psoap";
        else d = std::string("/tmp/psoap-") + std::to_string((long long)geteuid());
        if (mkdir(d.c_str(), 0700) != 0 && errno != EEXIST) return;
        struct stat sb;
        if (lstat(d.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode) || sb.st_uid != geteuid()) {
            fprintf(stderr, "psoap: %s is not a directory of this user: several processes on one GPU are not serialised\n", d.c_str());
            return;
        }
        dir = d;
    });
    return dir;
}

static std::string device_file(int device, const char* suffix)
{
    std::string bus = share_bus_id(device);
    if (bus.empty()) bus = "index" + std::to_string(device);
    for (char& c : bus)
        if (!((c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'))) c = '_';
    return share_dir() + "/gpu_" + bus + suffix;
}

static int open_share_file(const std::string& path, bool create)
{
    return open(path.c_str(), (create ? O_CREAT : 0) | O_RDWR | O_CLOEXEC | O_NOFOLLOW, 0600);
}

// 0: the device is this process's (*took), or no lock is needed -- switched off / unavailable, or this process runs the
// staged path on a device too many processes share (share_wants_staged: kernel boundaries only, nothing to keep apart, and
// 16 processes interleaving their kernels measured 143 evaluations per second at N = 6000 against 16 taking turns);
// 2: timed out (g_err says who holds it)
static bool share_wants_staged(int device);
static int device_lock_acquire(int device, bool* took = nullptr)
{
    if (took) *took = false;
    if (!device_lock_enabled()) return 0;
    if (share_wants_staged(device)) return 0;
    DeviceLock* Lp;
    {
        std::lock_guard<std::mutex> g(g_devlock_mu);
        Lp = &g_devlocks[device];          // (constructed in place; map nodes do not move)
    }
    DeviceLock& L = *Lp;
    std::unique_lock<std::mutex> lk(L.mu);
    if (L.pid != getpid()) {          // first use in this process (a descriptor inherited through fork() shares its lock)
        if (L.fd >= 0) (void)close(L.fd);
        L.fd = -1;
        L.refs = 0;
        L.held = L.acquiring = false;
        L.pid = getpid();
        if (!share_dir().empty()) {
            L.path = device_file(device, ".lock");
            L.fd = open_share_file(L.path, true);
        }
        if (L.fd < 0 && !L.broken) {
            L.broken = true;
            fprintf(stderr, "psoap: cannot open the device lock %s: several processes on this GPU are not serialised\n",
                    L.path.empty() ? "(no lock directory)" : L.path.c_str());
        }
    }
    if (L.fd < 0) return 0;
    ++L.refs;
    if (took) *took = true;
    if (L.held) return 0;
    if (L.acquiring) {                 // another thread of this process is at it: wait for its verdict
        L.cv.wait(lk, [&] { return !L.acquiring; });
        if (L.held) return 0;
        if (took) *took = false;
        --L.refs;
        g_err = "psoap: the device lock could not be taken (see the other thread's error)";
        return 2;
    }
    L.acquiring = true;
    const int fd = L.fd;
    lk.unlock();
    // (polled, not blocking: a wait that never ends must become an error.  20 us steps at first -- the holder's evaluation
    // takes milliseconds -- then 200 us.)
    const auto t0 = std::chrono::steady_clock::now();
    const double limit = device_lock_timeout_s();
    bool got = false;
    long long polls = 0;
    for (;;) {
        if (flock(fd, LOCK_EX | LOCK_NB) == 0) {
            got = true;
            break;
        }
        if (errno != EWOULDBLOCK && errno != EINTR) break;
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit) break;
        struct timespec ts = {0, (++polls < 200) ? 20000L : 200000L};
        (void)nanosleep(&ts, nullptr);
    }
    const long long waited_us =
        (long long)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (got) {
        char buf[32];
        const int n = snprintf(buf, sizeof buf, "%ld\n", (long)getpid());
        if (pwrite(fd, buf, (size_t)n, 0) == n) {      // who holds it (diagnostics of a time-out elsewhere)
            const int rc = ftruncate(fd, n);
            (void)rc;
        }
        g_share.lock_acquisitions += 1;
        g_share.lock_wait_us += waited_us;
    }
    lk.lock();
    L.acquiring = false;
    L.held = got;
    if (!got) --L.refs;
    L.cv.notify_all();
    if (!got) {
        if (took) *took = false;
        char who[32] = {0};
        const ssize_t n = pread(fd, who, sizeof who - 1, 0);
        for (ssize_t i = 0; i < n; ++i)
            if (who[i] == '\n') who[i] = 0;
        g_err = "psoap: the device lock " + L.path + " was not released within " + std::to_string((int)limit) +
                " s (PSOAP_DEVICE_LOCK_TIMEOUT_S); last holder: pid " + (n > 0 ? who : "unknown");
        return 2;
    }
    return 0;
}

static void device_lock_release(int device)
{
    if (!device_lock_enabled()) return;
    DeviceLock* Lp = nullptr;
    {
        std::lock_guard<std::mutex> g(g_devlock_mu);
        auto it = g_devlocks.find(device);
        if (it == g_devlocks.end()) return;
        Lp = &it->second;
    }
    std::lock_guard<std::mutex> lk(Lp->mu);
    if (Lp->fd < 0 || Lp->pid != getpid() || Lp->refs <= 0) return;
    if (--Lp->refs == 0 && Lp->held) {
        (void)flock(Lp->fd, LOCK_UN);
        Lp->held = false;
    }
}

// How many cooperating processes use a device: each holds one of 64 slot files (<dir>/gpu_<bus>.slot<k>, locked for the
// life of the process; PSOAP_DEVICE_SLOTS=0: no count).  Counted whether or not the lock is on: without the lock the count
// is what sends evaluations down the staged path.
struct SlotState {
    int fd = -1;
    pid_t pid = 0;
    int procs = 1;
    std::chrono::steady_clock::time_point counted{};
    bool warned = false;
};
static std::map<int, SlotState> g_slots;
static bool device_slots_enabled()
{
    static const bool on = !(getenv("PSOAP_DEVICE_SLOTS") && getenv("PSOAP_DEVICE_SLOTS")[0] == '0');
    return on;
}
static void device_slot_take(int device)
{
    if (!device_slots_enabled() || share_dir().empty()) return;
    std::lock_guard<std::mutex> g(g_devlock_mu);
    SlotState& S = g_slots[device];
    if (S.pid == getpid() && S.fd >= 0) return;
    if (S.fd >= 0) (void)close(S.fd);       // (inherited through fork(): shares its lock with the parent)
    S = SlotState();
    S.pid = getpid();
    for (int k = 0; k < 64; ++k) {
        const int fd = open_share_file(device_file(device, (".slot" + std::to_string(k)).c_str()), true);
        if (fd < 0) break;
        if (flock(fd, LOCK_EX | LOCK_NB) == 0) {
            S.fd = fd;
            break;
        }
        (void)close(fd);
    }
}
// The driver's own account of who uses the device: every process that has opened /dev/kfd appears under
// /sys/class/kfd/kfd/proc/<pid>/ with one entry per hardware queue (queues/<id>/gpuid).  Counting the processes with a queue
// on THIS device sees what the slot files cannot: programs that do not go through this library (a torch job, another
// user's work) -- they, too, take one of the eight process contexts the device keeps mapped.  -1 where sysfs does not say
// (no KFD, a container without it, PSOAP_KFD_COUNT=0).  The device's KFD id comes from the topology node whose PCI location
// matches share_bus_id.  `root`: the KFD tree (tests pass one of their own).
static int kfd_procs_on_device(int device, const std::string& root = "/sys/class/kfd/kfd")
{
    static const bool off = getenv("PSOAP_KFD_COUNT") && getenv("PSOAP_KFD_COUNT")[0] == '0';
    if (off) return -1;
    static std::map<int, std::string> gpu_ids;          // per HIP device: its KFD gpu_id ("" = unknown); guarded by g_devlock_mu
    auto it = gpu_ids.find(device);
    if (it == gpu_ids.end()) {
        std::string found;
        unsigned int dom = 0, b = 0, d = 0, f = 0;
        if (sscanf(share_bus_id(device).c_str(), "%x:%x:%x.%x", &dom, &b, &d, &f) == 4) {
            const unsigned long want_loc = ((unsigned long)b << 8) | ((unsigned long)d << 3) | (unsigned long)f;
            if (DIR* nodes = opendir((root + "/topology/nodes").c_str())) {
                while (struct dirent* e = readdir(nodes)) {
                    if (e->d_name[0] == '.') continue;
                    const std::string nd = root + "/topology/nodes/" + e->d_name;
                    FILE* fp = fopen((nd + "/properties").c_str(), "r");
                    if (!fp) continue;
                    char key[64];
                    unsigned long long val = 0, loc = ~0ull, domain = 0, simd = 0;
                    while (fscanf(fp, "%63s %llu", key, &val) == 2) {
                        if (!strcmp(key, "location_id")) loc = val;
                        else if (!strcmp(key, "domain")) domain = val;
                        else if (!strcmp(key, "simd_count")) simd = val;
                    }
                    fclose(fp);
                    if (simd == 0 || loc != want_loc || domain != dom) continue;
                    if (FILE* fg = fopen((nd + "/gpu_id").c_str(), "r")) {
                        char id[32] = {0};
                        if (fscanf(fg, "%31s", id) == 1) found = id;
                        fclose(fg);
                    }
                }
                closedir(nodes);
            }
        }
        it = gpu_ids.emplace(device, found).first;
    }
    if (it->second.empty()) return -1;
    DIR* procs = opendir((root + "/proc").c_str());
    if (!procs) return -1;
    int n = 0;
    while (struct dirent* e = readdir(procs)) {
        if (e->d_name[0] < '0' || e->d_name[0] > '9') continue;
        const std::string qd = root + "/proc/" + e->d_name + "/queues";
        DIR* qs = opendir(qd.c_str());
        if (!qs) continue;
        bool here = false;
        while (struct dirent* q = readdir(qs)) {
            if (q->d_name[0] == '.' || here) continue;
            if (FILE* fg = fopen((qd + "/" + q->d_name + "/gpuid").c_str(), "r")) {
                char id[32] = {0};
                if (fscanf(fg, "%31s", id) == 1 && it->second == id) here = true;
                fclose(fg);
            }
        }
        closedir(qs);
        n += here ? 1 : 0;
    }
    closedir(procs);
    return n;
}

// processes on this device: those with a slot file (this library's), or -- where the driver says -- all that hold a hardware
// queue on it (kfd_procs_on_device), whichever is more; this one included; re-counted at most four times a second
static int share_procs(int device)
{
    if (const char* e = getenv("PSOAP_SHARE_PROCS"))      // tests: pretend
        if (atoi(e) > 0) return atoi(e);
    if (!device_slots_enabled() || share_dir().empty()) return 1;
    std::lock_guard<std::mutex> g(g_devlock_mu);
    SlotState& S = g_slots[device];
    if (S.pid != getpid() || S.fd < 0) return 1;
    const auto now = std::chrono::steady_clock::now();
    if (S.counted.time_since_epoch().count() != 0 && std::chrono::duration<double>(now - S.counted).count() < 0.25) return S.procs;
    int n = 0;
    for (int k = 0; k < 64; ++k) {
        const int fd = open_share_file(device_file(device, (".slot" + std::to_string(k)).c_str()), false);
        if (fd < 0) break;                              // slot files are created in order and never removed
        if (flock(fd, LOCK_EX | LOCK_NB) == 0) (void)flock(fd, LOCK_UN);
        else ++n;                                       // held: by another process, or by this one's own descriptor
        (void)close(fd);
    }
    const int k = kfd_procs_on_device(device);
    if (k > n) n = k;
    S.procs = n > 0 ? n : 1;
    S.counted = now;
    return S.procs;
}

// Which path an evaluation takes on a device that `procs` processes share.
static int share_dag_max()
{
    const char* e = getenv("PSOAP_SHARE_DAG_MAX");
    return (e && atoi(e) > 0) ? atoi(e) : 8;
}
static int share_retries()
{
    const char* e = getenv("PSOAP_SHARE_RETRIES");
    return (e && atoi(e) >= 0) ? atoi(e) : 3;
}
// experiments (tools/shared_gpu_probe.py): disturbed launches are counted but their values handed out all the same -- is
// every wrong value one of a launch that reported a moved workgroup?
static bool share_detect_only()
{
    static const bool on = getenv("PSOAP_SHARE_DETECT_ONLY") && getenv("PSOAP_SHARE_DETECT_ONLY")[0] == '1';
    return on;
}
// The decision is taken ONCE per entry into the library and kept for the whole call (DeviceScope below): the process count
// is re-read four times a second, and a call that asked twice -- once to decide whether it needs the device lock, once to
// choose the path -- could get two answers: a persistent launch issued WITHOUT the lock (review of round 5).
static thread_local int g_share_decision_depth = 0;       // > 0: inside an entry point
static thread_local std::map<int, bool>* g_share_decision = nullptr;
static bool share_wants_staged_now(int device);
static bool share_wants_staged(int device)
{
    if (g_share_decision_depth > 0 && g_share_decision) {
        auto it = g_share_decision->find(device);
        if (it != g_share_decision->end()) return it->second;
        const bool v = share_wants_staged_now(device);
        (*g_share_decision)[device] = v;
        return v;
    }
    return share_wants_staged_now(device);
}
static void share_warn_unsafe_regime(int procs, bool pinned_dag);
static bool share_wants_staged_now(int device)
{
    static const int pinned = [] {
        const char* e = getenv("PSOAP_SHARE_POLICY");
        return !e ? 0 : (!strcmp(e, "dag") ? 1 : (!strcmp(e, "staged") ? 2 : 0));
    }();
    if (pinned) {
        if (pinned == 1) share_warn_unsafe_regime(share_procs(device), true);
        return pinned == 2;
    }
    const int procs = share_procs(device);
    if (procs <= 1) return false;
    if (!device_lock_enabled()) return true;            // nobody keeps two persistent launches apart
    if (procs <= share_dag_max()) {
        share_warn_unsafe_regime(procs, false);
        return false;
    }
    static std::atomic<bool> hinted{false};
    if (!hinted.exchange(true) && !(getenv("PSOAP_QUIET") && getenv("PSOAP_QUIET")[0] == '1'))
        fprintf(stderr,
                "psoap: %d processes share this GPU: evaluations take the staged path (safe, slower).  PSOAP_GPU_SERVER=auto lets "
                "ONE process own the device and evaluate all workers' calls in group launches (psoap_amd/server.py: 4-9 x the "
                "rate beyond 8 workers).\n", procs);
    return true;
}
// tests: every k-th launch is treated as tainted (PSOAP_TEST_TAINT_EVERY=k), to drive the retry / fallback logic on a
// device nobody shares
static bool share_inject_taint()
{
    static const int every = getenv("PSOAP_TEST_TAINT_EVERY") ? atoi(getenv("PSOAP_TEST_TAINT_EVERY")) : 0;
    static std::atomic<long long> n{0};
    return every > 0 && (++n % every) == 0;
}

// Persistent launches among MORE than 8 process contexts are outside what was measured clean: a user who pins
// them there (PSOAP_SHARE_POLICY=dag, PSOAP_SHARE_DAG_MAX > 8) or asks for tainted values (PSOAP_SHARE_DETECT_ONLY=1) is told
// so, once.
static void share_warn_unsafe_regime(int procs, bool pinned_dag)
{
    static std::atomic<bool> warned{false};
    const bool beyond = procs > 8 && (pinned_dag || share_dag_max() > 8);
    if (!(beyond || share_detect_only()) || warned.exchange(true)) return;
    if (getenv("PSOAP_QUIET") && getenv("PSOAP_QUIET")[0] == '1') return;
    if (share_detect_only())
        fprintf(stderr, "psoap: PSOAP_SHARE_DETECT_ONLY=1: evaluations that reported a moved workgroup are handed out as they are "
                        "(an experiment's setting: such values may be wrong).\n");
    if (beyond)
        fprintf(stderr, "psoap: %d processes share this GPU and the persistent kernel was pinned there (PSOAP_SHARE_POLICY=dag or "
                        "PSOAP_SHARE_DAG_MAX > 8): the moved-workgroup check was measured clean only up to 8 processes; beyond, "
                        "the staged path or PSOAP_GPU_SERVER=auto is the supported route.\n", procs);
}

struct DeviceScope {
    int dev;
    bool ok, took = false;
    std::map<int, bool> decisions;          // share_wants_staged per device, fixed for the duration of this call
    bool outermost = false;
    explicit DeviceScope(int d) : dev(d)
    {
        if (g_share_decision_depth++ == 0) {
            g_share_decision = &decisions;
            outermost = true;
        }
        ok = device_lock_acquire(d, &took) == 0;
    }
    ~DeviceScope()
    {
        if (took) device_lock_release(dev);
        if (--g_share_decision_depth == 0 && outermost) g_share_decision = nullptr;
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};
// every entry point that touches the device: the lock for the duration of the call, an error when it cannot be had
#define DEVICE_SCOPE(d)      \
    DeviceScope scope_(d);   \
    if (!scope_.ok) return 2
// the destroy entry points: the resources go whether or not the lock could be had (a time-out there must not leak device
// memory, nor make the caller's close() raise: a device-wide synchronise and freeing memory disturb nobody's persistent launch)
#define DEVICE_SCOPE_DESTROY(d) DeviceScope scope_(d)
