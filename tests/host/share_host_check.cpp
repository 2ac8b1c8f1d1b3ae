// share_host_check.cpp -- the device-sharing layer (psoap_amd/csrc/share.hpp) as a stand-alone host program: no HIP header,
// no HIP library, no GPU, no /sys.  tests/test_share_host.py builds it with AddressSanitizer and UBSan (the `threads` mode
// with ThreadSanitizer as well) and runs it once per mode: several settings are read once per process, so every mode gets a
// process -- and an environment, a lock directory -- of its own.  The program checks its own expectations and leaves with
// status 1 and a line on stderr at the first that fails; what the layer itself prints on stderr is the caller's to check.
//     share_host_check MODE [SCRATCH_DIR]
// Other processes are forked children that report through a pipe and leave when told to: nobody sleeps except for the
// 0.25 s recount interval of share_procs and the 0.3 s lock time-outs.
// (Not covered: a lock directory that belongs to ANOTHER user -- share_dir's st_uid check -- cannot be made without root.)
#include <signal.h>
#include <sys/wait.h>

#include <functional>
#include <thread>
#include <vector>

#include "../../psoap_amd/csrc/share.hpp"

// devices of this program: A, B, none, A's location in domain 1, behind an over-long key, behind a non-numeric value, behind
// a 63-character key, no node, malformed, A again (for a second tree: the KFD id of a device is looked up once)
enum { DEV_A = 0, DEV_B, DEV_NONE, DEV_C, DEV_LONGKEY, DEV_TEXT, DEV_KEY63, DEV_NO_NODE, DEV_MALFORMED, DEV_A_AGAIN, N_DEV };
static std::string share_bus_id(int device)
{
    static const char* const ids[N_DEV] = {"0000:c1:00.0", "0000:05:00.0", "",           "0001:c1:00.0", "0000:07:00.0",
                                           "0000:08:00.0", "0000:09:00.0", "0000:ff:00.0", "c1-00-0",      "0000:c1:00.0"};
    return device >= 0 && device < N_DEV ? ids[device] : "";
}

static const char* g_mode = "?";
static std::vector<pid_t> g_children;

[[noreturn]] static void die(int line, const char* expr)
{
    fprintf(stderr, "share_host_check %s: line %d: expected %s (pid %ld, last error: %s)\n", g_mode, line, expr, (long)getpid(),
            g_err.c_str());
    fflush(stderr);
    for (pid_t p : g_children) (void)kill(p, SIGKILL);
    _exit(1);
}
#define EXPECT(c)                      \
    do {                               \
        if (!(c)) die(__LINE__, #c);   \
    } while (0)

// ---- other processes ------------------------------------------------------------------------------------------------
struct Child {
    pid_t pid = -1;
    int to = -1, from = -1;
    bool told()                        // the child's next report; false: it left without one
    {
        char c;
        ssize_t n;
        while ((n = read(from, &c, 1)) < 0 && errno == EINTR) {}
        return n == 1;
    }
    void go() { EXPECT(write(to, "g", 1) == 1); }
    int finish()                       // its exit status, -1: it did not exit
    {
        int st = 0;
        (void)close(to);
        (void)close(from);
        EXPECT(waitpid(pid, &st, 0) == pid);
        return WIFEXITED(st) ? WEXITSTATUS(st) : -1;
    }
};
// body(tell, wait_go) runs in a forked child, which leaves with status 0 after it (an EXPECT that fails there: 1)
static Child spawn(const std::function<void(const std::function<void()>&, const std::function<void()>&)>& body)
{
    int down[2], up[2];
    EXPECT(pipe(down) == 0 && pipe(up) == 0);
    fflush(stdout);
    const pid_t p = fork();
    EXPECT(p >= 0);
    if (p == 0) {
        g_children.clear();
        (void)alarm(30);               // whatever happens to the parent, nothing stays behind
        (void)close(down[1]);
        (void)close(up[0]);
        body([&] { EXPECT(write(up[1], "t", 1) == 1); },
             [&] {
                 char c;
                 while (read(down[0], &c, 1) < 0 && errno == EINTR) {}
             });
        _exit(0);
    }
    (void)close(down[0]);
    (void)close(up[1]);
    g_children.push_back(p);
    Child c;
    c.pid = p;
    c.to = down[1];
    c.from = up[0];
    return c;
}

// can ANOTHER process take the flock on this file right now?
static bool flock_free(const std::string& path)
{
    Child c = spawn([&](const std::function<void()>&, const std::function<void()>&) {
        const int fd = open(path.c_str(), O_RDWR | O_CLOEXEC);
        if (fd < 0) _exit(2);
        _exit(flock(fd, LOCK_EX | LOCK_NB) == 0 ? 0 : 3);
    });
    const int st = c.finish();
    EXPECT(st == 0 || st == 3);
    return st == 0;
}

// ---- what the files look like --------------------------------------------------------------------------------------
static int file_mode(const std::string& path)            // permission bits, -1: not there; never through a symlink
{
    struct stat sb;
    return lstat(path.c_str(), &sb) == 0 ? (int)(sb.st_mode & 07777) : -1;
}
static bool is_kind(const std::string& path, mode_t kind)
{
    struct stat sb;
    return lstat(path.c_str(), &sb) == 0 && (sb.st_mode & S_IFMT) == kind;
}
static std::string slurp(const std::string& path)
{
    std::string s;
    if (FILE* f = fopen(path.c_str(), "r")) {
        char buf[256];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
        fclose(f);
    }
    return s;
}
static void spit(const std::string& path, const std::string& text)
{
    FILE* f = fopen(path.c_str(), "w");
    EXPECT(f != nullptr);
    EXPECT(fwrite(text.data(), 1, text.size(), f) == text.size());
    EXPECT(fclose(f) == 0);
}
static void mkdirs(const std::string& path)
{
    for (size_t i = 1; i <= path.size(); ++i)
        if (i == path.size() || path[i] == '/') EXPECT(mkdir(path.substr(0, i).c_str(), 0700) == 0 || errno == EEXIST);
}
static ino_t inode_of_path(const std::string& path)
{
    struct stat sb;
    EXPECT(stat(path.c_str(), &sb) == 0);
    return sb.st_ino;
}
static ino_t inode_of_fd(int fd)
{
    struct stat sb;
    EXPECT(fstat(fd, &sb) == 0);
    return sb.st_ino;
}
static int lock_refs(int device)
{
    std::lock_guard<std::mutex> g(g_devlock_mu);
    auto it = g_devlocks.find(device);
    if (it == g_devlocks.end()) return 0;
    std::lock_guard<std::mutex> lk(it->second.mu);
    return it->second.refs;
}
static double seconds_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
static void sleep_past_recount()
{
    struct timespec ts = {0, 270000000L};                 // share_procs counts again after 0.25 s
    while (nanosleep(&ts, &ts) != 0 && errno == EINTR) {}
}
static void pretend_procs(int n)
{
    if (n > 0) EXPECT(setenv("PSOAP_SHARE_PROCS", std::to_string(n).c_str(), 1) == 0);
    else EXPECT(unsetenv("PSOAP_SHARE_PROCS") == 0);
}
static std::string lock_dir()
{
    const char* e = getenv("PSOAP_LOCK_DIR");
    EXPECT(e != nullptr);
    return e;
}

// ---- dir: a missing directory is made 0700; the files are 0600 and named after the bus id ----------------------------
static void mode_dir()
{
    const std::string d = lock_dir();
    EXPECT(file_mode(d) == -1);
    EXPECT(share_dir() == d);
    EXPECT(is_kind(d, S_IFDIR) && file_mode(d) == 0700);
    bool took = false;
    EXPECT(device_lock_acquire(DEV_A, &took) == 0 && took);
    EXPECT(is_kind(d + "/gpu_0000_c1_00_0.lock", S_IFREG) && file_mode(d + "/gpu_0000_c1_00_0.lock") == 0600);
    device_slot_take(DEV_A);
    EXPECT(is_kind(d + "/gpu_0000_c1_00_0.slot0", S_IFREG) && file_mode(d + "/gpu_0000_c1_00_0.slot0") == 0600);
    EXPECT(file_mode(d + "/gpu_0000_c1_00_0.slot1") == -1);
    device_lock_release(DEV_A);
    EXPECT(device_lock_acquire(DEV_B, &took) == 0 && took);
    EXPECT(file_mode(d + "/gpu_0000_05_00_0.lock") == 0600);
    device_lock_release(DEV_B);
    EXPECT(device_lock_acquire(DEV_NONE, &took) == 0 && took);          // no bus id: the device's index
    EXPECT(file_mode(d + "/gpu_index2.lock") == 0600);
    device_lock_release(DEV_NONE);
    EXPECT(device_file(DEV_MALFORMED, ".slot12") == d + "/gpu_c1_00_0.slot12");
}

// ---- dir-symlink, dir-file: no directory of this user, no lock, said once (each of the two lines) ---------------------
static void mode_no_dir()
{
    EXPECT(file_mode(lock_dir()) != -1 && !is_kind(lock_dir(), S_IFDIR));
    for (int k = 0; k < 3; ++k) {
        bool took = true;
        EXPECT(share_dir().empty());
        EXPECT(device_lock_acquire(DEV_A, &took) == 0 && !took);
        device_lock_release(DEV_A);
        device_slot_take(DEV_A);
        EXPECT(share_procs(DEV_A) == 1);
    }
    EXPECT(g_share.lock_acquisitions.load() == 0);
}

// ---- lock-symlink: a lock file that is a symlink is not followed; said once, not on every acquire ----------------------
static void mode_lock_symlink()
{
    const std::string d = lock_dir();
    spit(d + "/elsewhere", "");
    EXPECT(symlink((d + "/elsewhere").c_str(), (d + "/gpu_0000_c1_00_0.lock").c_str()) == 0);
    for (int k = 0; k < 3; ++k) {
        bool took = true;
        EXPECT(device_lock_acquire(DEV_A, &took) == 0 && !took);
        device_lock_release(DEV_A);
    }
    EXPECT(slurp(d + "/elsewhere").empty());
    bool took = false;                                     // the other devices' locks are none the worse
    EXPECT(device_lock_acquire(DEV_B, &took) == 0 && took);
    device_lock_release(DEV_B);
}

// ---- lock: counted within the process, held until the last release ------------------------------------------------
static void mode_lock()
{
    const std::string path = lock_dir() + "/gpu_0000_c1_00_0.lock";
    device_lock_release(DEV_A);                            // nothing acquired yet: nothing happens
    bool took = false;
    EXPECT(device_lock_acquire(DEV_A, &took) == 0 && took);
    EXPECT(device_lock_acquire(DEV_A, &took) == 0 && took);
    EXPECT(lock_refs(DEV_A) == 2);
    EXPECT(slurp(path) == std::to_string((long)getpid()) + "\n");
    EXPECT(!flock_free(path));
    device_lock_release(DEV_A);
    EXPECT(!flock_free(path));
    device_lock_release(DEV_A);
    EXPECT(flock_free(path));
    EXPECT(g_share.lock_acquisitions.load() == 1);
    device_lock_release(DEV_A);                            // one release too many: nothing happens
    EXPECT(lock_refs(DEV_A) == 0);
    EXPECT(device_lock_acquire(DEV_A) == 0);               // (no `took`: the callers that hold it until a later call)
    EXPECT(lock_refs(DEV_A) == 1 && !flock_free(path));
    device_lock_release(DEV_A);
    EXPECT(flock_free(path));
    EXPECT(g_share.lock_acquisitions.load() == 2);
    EXPECT(slurp(path) == std::to_string((long)getpid()) + "\n");
}

// ---- timeout (PSOAP_DEVICE_LOCK_TIMEOUT_S=0.3): another process holds the lock --------------------------------------
static Child holder_of(int device)
{
    Child c = spawn([&](const std::function<void()>& tell, const std::function<void()>& wait_go) {
        bool took = false;
        EXPECT(device_lock_acquire(device, &took) == 0 && took);
        tell();
        wait_go();
        device_lock_release(device);
    });
    EXPECT(c.told());
    return c;
}
static void mode_timeout()
{
    const std::string path = lock_dir() + "/gpu_0000_c1_00_0.lock";
    EXPECT(device_lock_timeout_s() == 0.3);
    Child c = holder_of(DEV_A);
    bool took = true;
    const auto t0 = std::chrono::steady_clock::now();
    EXPECT(device_lock_acquire(DEV_A, &took) == 2 && !took);
    const double waited = seconds_since(t0);
    EXPECT(waited >= 0.3 && waited < 5.0);                 // (the upper figure only catches a hang: the poll step is 200 us)
    EXPECT(g_err.find("last holder: pid " + std::to_string((long)c.pid)) != std::string::npos);
    EXPECT(g_err.find(path) != std::string::npos);
    EXPECT(g_err.find("was not released within 0 s ") != std::string::npos);      // as it is today: whole seconds, 0.3 -> 0
    EXPECT(lock_refs(DEV_A) == 0);
    EXPECT(g_share.lock_acquisitions.load() == 0);
    c.go();
    EXPECT(c.finish() == 0);
    EXPECT(device_lock_acquire(DEV_A, &took) == 0 && took);
    EXPECT(lock_refs(DEV_A) == 1 && !flock_free(path));
    device_lock_release(DEV_A);
    EXPECT(flock_free(path));
}

// ---- fork (PSOAP_DEVICE_LOCK_TIMEOUT_S=0.3): a child starts over, with descriptors of its own -----------------------
static void mode_fork()
{
    const std::string d = lock_dir();
    bool took = false;
    EXPECT(device_lock_acquire(DEV_A, &took) == 0 && took);
    device_slot_take(DEV_A);
    EXPECT(inode_of_fd(g_slots[DEV_A].fd) == inode_of_path(d + "/gpu_0000_c1_00_0.slot0"));
    Child c = spawn([&](const std::function<void()>& tell, const std::function<void()>& wait_go) {
        bool mine = true;
        EXPECT(device_lock_acquire(DEV_A, &mine) == 2 && !mine);        // not inherited: the parent holds it
        EXPECT(lock_refs(DEV_A) == 0);
        device_slot_take(DEV_A);                                         // nor the parent's slot
        EXPECT(g_slots[DEV_A].pid == getpid());
        EXPECT(inode_of_fd(g_slots[DEV_A].fd) == inode_of_path(d + "/gpu_0000_c1_00_0.slot1"));
        tell();
        wait_go();
        EXPECT(device_lock_acquire(DEV_A, &mine) == 0 && mine);
        EXPECT(slurp(d + "/gpu_0000_c1_00_0.lock") == std::to_string((long)getpid()) + "\n");
        tell();
        wait_go();
        device_lock_release(DEV_A);
    });
    EXPECT(c.told());
    EXPECT(!flock_free(d + "/gpu_0000_c1_00_0.lock"));                   // the child's time-out released nothing of the parent's
    device_lock_release(DEV_A);
    c.go();
    EXPECT(c.told());
    EXPECT(device_lock_acquire(DEV_A, &took) == 2 && !took);            // now the child holds it
    EXPECT(g_err.find("last holder: pid " + std::to_string((long)c.pid)) != std::string::npos);
    c.go();
    EXPECT(c.finish() == 0);
    EXPECT(inode_of_fd(g_slots[DEV_A].fd) == inode_of_path(d + "/gpu_0000_c1_00_0.slot0"));
    EXPECT(flock_free(d + "/gpu_0000_c1_00_0.slot1") && !flock_free(d + "/gpu_0000_c1_00_0.slot0"));
}

// ---- slots: the count of the processes that hold a slot file, taken again after 0.25 s -------------------------------
static void mode_slots()
{
    const std::string d = lock_dir();
    EXPECT(share_procs(DEV_A) == 1);                       // no slot yet: not counted at all
    device_slot_take(DEV_A);
    EXPECT(share_procs(DEV_A) == 1);                       // k = 0 (the first count is taken at once)
    for (int k : {1, 3}) {
        std::vector<Child> cs;
        for (int i = 0; i < k; ++i) {
            cs.push_back(spawn([&](const std::function<void()>& tell, const std::function<void()>& wait_go) {
                device_slot_take(DEV_A);
                EXPECT(g_slots[DEV_A].fd >= 0);
                tell();
                wait_go();
            }));
            EXPECT(cs.back().told());
        }
        sleep_past_recount();
        EXPECT(share_procs(DEV_A) == k + 1);
        const auto counted = std::chrono::steady_clock::now();
        EXPECT(share_procs(DEV_B) == 1);                   // another device: this process has no slot there
        for (Child& c : cs) {
            c.go();
            EXPECT(c.finish() == 0);
        }
        const int again = share_procs(DEV_A);              // within the interval: the count that was taken
        EXPECT(again == k + 1 || seconds_since(counted) >= 0.2);
    }
    EXPECT(file_mode(d + "/gpu_0000_c1_00_0.slot3") == 0600 && file_mode(d + "/gpu_0000_c1_00_0.slot4") == -1);
    pretend_procs(5);
    EXPECT(share_procs(DEV_A) == 5 && share_procs(DEV_NO_NODE) == 5);
    pretend_procs(0);
    sleep_past_recount();
    EXPECT(share_procs(DEV_A) == 1);                       // the files stay, nobody holds them
}
// PSOAP_DEVICE_SLOTS=0: no files, no count
static void mode_slots_off()
{
    Child c = spawn([&](const std::function<void()>& tell, const std::function<void()>& wait_go) {
        device_slot_take(DEV_A);
        tell();
        wait_go();
    });
    EXPECT(c.told());
    device_slot_take(DEV_A);
    EXPECT(share_procs(DEV_A) == 1);
    EXPECT(file_mode(lock_dir() + "/gpu_0000_c1_00_0.slot0") == -1);
    c.go();
    EXPECT(c.finish() == 0);
    pretend_procs(5);
    EXPECT(share_procs(DEV_A) == 5);
}

// ---- kfd: the driver's tree, as this program writes it ------------------------------------------------------------
static void kfd_node(const std::string& root, int k, const std::string& properties, const std::string& gpu_id)
{
    const std::string nd = root + "/topology/nodes/" + std::to_string(k);
    mkdirs(nd);
    spit(nd + "/properties", properties);
    spit(nd + "/gpu_id", gpu_id);
}
static void kfd_queue(const std::string& root, const std::string& pid, int q, const std::string& gpuid)
{
    const std::string qd = root + "/proc/" + pid + "/queues/" + std::to_string(q);
    mkdirs(qd);
    spit(qd + "/gpuid", gpuid);
}
static std::string gpu_props(unsigned long location_id, unsigned long domain, const std::string& before_location = "")
{
    return "cpu_cores_count 0\nsimd_count 1024\n" + before_location + "location_id " + std::to_string(location_id) + "\ndomain " +
           std::to_string(domain) + "\nmax_engine_clk_fcompute 2400\n";
}
static void mode_kfd(const std::string& scratch)
{
    const std::string root = scratch + "/kfd";
    // location_id = bus << 8 | device << 3 | function
    kfd_node(root, 0, "cpu_cores_count 64\nsimd_count 0\nlocation_id 0\ndomain 0\n", "0\n");
    kfd_node(root, 1, gpu_props(0xc100, 0), "51234\n");                                       // A
    kfd_node(root, 2, gpu_props(0x0500, 0), "7777\n");                                        // B
    kfd_node(root, 3, "", "4242\n");                                                          // says nothing
    kfd_node(root, 4, gpu_props(0xc100, 1), "999\n");                                         // A's location, domain 1
    kfd_node(root, 5, gpu_props(0x0700, 0, std::string(64, 'k') + " 1\n"), "64064\n");
    kfd_node(root, 6, gpu_props(0x0800, 0, "vendor_name AMD\n"), "8080\n");
    kfd_node(root, 7, gpu_props(0x0900, 0, std::string(63, 'k') + " 1\n"), "63063\n");
    kfd_queue(root, "100", 0, "51234\n");                  // two queues on A: one process
    kfd_queue(root, "100", 1, "51234\n");
    kfd_queue(root, "200", 0, "51234\n");                  // one on A, one on B
    kfd_queue(root, "200", 1, "7777\n");
    mkdirs(root + "/proc/300/queues");                     // has opened the driver, holds no queue
    kfd_queue(root, "400", 0, "");                         // a queue that does not say where
    kfd_queue(root, "self", 0, "51234\n");                 // not a pid
    kfd_queue(root, "500", 0, "63063\n");
    kfd_queue(root, "500", 1, "64064\n");
    kfd_queue(root, "500", 2, "8080\n");
    EXPECT(kfd_procs_on_device(DEV_A, root) == 2);
    EXPECT(kfd_procs_on_device(DEV_B, root) == 1);
    EXPECT(kfd_procs_on_device(DEV_C, root) == 0);         // known to the driver, nobody on it
    EXPECT(kfd_procs_on_device(DEV_NO_NODE, root) == -1);
    EXPECT(kfd_procs_on_device(DEV_MALFORMED, root) == -1);
    EXPECT(kfd_procs_on_device(DEV_NONE, root) == -1);
    // What the parser does with lines it was not written for, as it is today: a key of 63 characters is read whole and the
    // file goes on; one of 64 is cut at 63, its last character is then no number, and THE REST OF THE FILE IS NOT READ -- nor
    // after a value that is no number.  A node whose location_id stands behind such a line is not found.
    EXPECT(kfd_procs_on_device(DEV_KEY63, root) == 1);
    EXPECT(kfd_procs_on_device(DEV_LONGKEY, root) == -1);
    EXPECT(kfd_procs_on_device(DEV_TEXT, root) == -1);
    EXPECT(kfd_procs_on_device(DEV_A, root) == 2);         // (the second time: the device's KFD id is remembered)
    // a tree without proc/
    const std::string bare = scratch + "/kfd_bare";
    kfd_node(bare, 0, gpu_props(0xc100, 0), "51234\n");
    EXPECT(kfd_procs_on_device(DEV_A_AGAIN, bare) == -1);
}
// PSOAP_KFD_COUNT=0
static void mode_kfd_off(const std::string& scratch)
{
    const std::string root = scratch + "/kfd";
    kfd_node(root, 1, gpu_props(0xc100, 0), "51234\n");
    kfd_queue(root, "100", 0, "51234\n");
    EXPECT(kfd_procs_on_device(DEV_A, root) == -1);
}

// ---- policy: which path, decided once per call ----------------------------------------------------------------------
static void check_memo(bool staged_at_9)
{
    // inside one scope the first answer for a device stands; a second device gets its own; afterwards: afresh
    pretend_procs(9);
    {
        DeviceScope outer(DEV_A);
        EXPECT(outer.ok && outer.took == !staged_at_9);
        pretend_procs(1);
        EXPECT(share_wants_staged(DEV_A) == staged_at_9);
        EXPECT(share_wants_staged_now(DEV_A) == false);
        {
            DeviceScope inner(DEV_A);
            EXPECT(inner.ok && inner.took == !staged_at_9 && !inner.outermost);
            EXPECT(share_wants_staged(DEV_B) == false);
        }
        EXPECT(g_share_decision == &outer.decisions && outer.decisions.size() == 2);
        pretend_procs(9);
        EXPECT(share_wants_staged(DEV_B) == false);
        EXPECT(share_wants_staged(DEV_A) == staged_at_9);
    }
    EXPECT(g_share_decision == nullptr && g_share_decision_depth == 0);
    EXPECT(share_wants_staged(DEV_B) == staged_at_9);
    pretend_procs(1);
    EXPECT(share_wants_staged(DEV_A) == false);
    EXPECT(lock_refs(DEV_A) == 0 && lock_refs(DEV_B) == 0);
}
static void mode_policy()
{
    const std::string path = lock_dir() + "/gpu_0000_c1_00_0.lock";
    EXPECT(share_dag_max() == 8 && share_retries() == 3 && !share_detect_only());
    for (int k = 0; k < 5; ++k) EXPECT(!share_inject_taint());
    pretend_procs(1);
    EXPECT(!share_wants_staged(DEV_A));
    for (int n = 2; n <= 8; ++n) {
        pretend_procs(n);
        EXPECT(!share_wants_staged(DEV_A));                // the lock keeps the persistent launches apart
    }
    pretend_procs(9);
    EXPECT(share_wants_staged(DEV_A));                     // the hint: here, once
    EXPECT(share_wants_staged(DEV_B));
    bool took = true;
    EXPECT(device_lock_acquire(DEV_A, &took) == 0 && !took);            // the staged path runs without the lock
    EXPECT(setenv("PSOAP_SHARE_DAG_MAX", "64", 1) == 0);
    pretend_procs(16);
    EXPECT(share_dag_max() == 64);
    EXPECT(!share_wants_staged(DEV_A));                    // the warning: here, once
    EXPECT(!share_wants_staged(DEV_A));
    pretend_procs(65);
    EXPECT(share_wants_staged(DEV_A));
    EXPECT(unsetenv("PSOAP_SHARE_DAG_MAX") == 0);
    EXPECT(setenv("PSOAP_SHARE_RETRIES", "0", 1) == 0 && share_retries() == 0);
    EXPECT(setenv("PSOAP_SHARE_RETRIES", "-1", 1) == 0 && share_retries() == 3);
    check_memo(true);
    // a scope whose acquire timed out: not ok, and it releases nothing
    pretend_procs(0);
    EXPECT(setenv("PSOAP_DEVICE_LOCK_TIMEOUT_S", "0.3", 1) == 0);
    Child c = holder_of(DEV_A);
    {
        DeviceScope s(DEV_A);
        EXPECT(!s.ok && !s.took);
        EXPECT(g_err.find("last holder: pid " + std::to_string((long)c.pid)) != std::string::npos);
    }
    EXPECT(lock_refs(DEV_A) == 0 && !flock_free(path));
    EXPECT(g_share_decision == nullptr && g_share_decision_depth == 0);
    c.go();
    EXPECT(c.finish() == 0);
    EXPECT(flock_free(path));
}
// PSOAP_DEVICE_LOCK=0: nobody keeps two persistent launches apart
static void mode_policy_nolock()
{
    pretend_procs(1);
    EXPECT(!share_wants_staged(DEV_A));
    for (int n = 2; n <= 9; ++n) {
        pretend_procs(n);
        EXPECT(share_wants_staged(DEV_A));
    }
    bool took = true;
    pretend_procs(1);
    EXPECT(device_lock_acquire(DEV_A, &took) == 0 && !took);
    device_lock_release(DEV_A);
    EXPECT(file_mode(lock_dir() + "/gpu_0000_c1_00_0.lock") == -1);
    EXPECT(g_devlocks.empty());
}
// PSOAP_SHARE_POLICY=dag | staged
static void mode_policy_pinned(bool staged)
{
    for (int n : {1, 2, 9, 100}) {
        pretend_procs(n);
        EXPECT(share_wants_staged(DEV_A) == staged);       // (dag, 9: the warning, once)
    }
    bool took = staged;
    EXPECT(device_lock_acquire(DEV_A, &took) == 0 && took == !staged);
    if (took) device_lock_release(DEV_A);
    if (!staged) check_memo(false);
}
// PSOAP_SHARE_DETECT_ONLY=1 PSOAP_TEST_TAINT_EVERY=3
static void mode_knobs()
{
    EXPECT(share_detect_only());
    for (int k = 1; k <= 9; ++k) EXPECT(share_inject_taint() == (k % 3 == 0));
    pretend_procs(2);
    EXPECT(!share_wants_staged(DEV_A));                    // (the detect-only warning: here, once)
    EXPECT(!share_wants_staged(DEV_A));
}

// ---- threads: eight threads and another process -----------------------------------------------------------------------
static void mode_threads()
{
    const std::string d = lock_dir();
    EXPECT(device_lock_timeout_s() == 300.0);
    Child c = spawn([&](const std::function<void()>& tell, const std::function<void()>& wait_go) {
        tell();
        wait_go();
        for (int k = 0; k < 5; ++k) {
            bool took = false;
            EXPECT(device_lock_acquire(DEV_A, &took) == 0 && took);
            struct timespec ts = {0, 1000000L};
            (void)nanosleep(&ts, nullptr);
            device_lock_release(DEV_A);
            (void)nanosleep(&ts, nullptr);
        }
    });
    EXPECT(c.told());
    device_slot_take(DEV_A);
    device_slot_take(DEV_B);
    std::atomic<int> errors{0}, rounds{0};
    std::vector<std::thread> ts;
    c.go();
    for (int t = 0; t < 8; ++t)
        ts.emplace_back([&, t] {
            for (int r = 0; r < 200; ++r) {
                const int dev = (t + r) % 2 ? DEV_B : DEV_A;
                if (r % 4 == 3) {                          // as an entry point does it, one inside another
                    DeviceScope outer(dev);
                    DeviceScope inner(dev);
                    if (!outer.ok || !inner.ok || !outer.took || !inner.took || share_wants_staged(dev)) errors += 1;
                } else {
                    bool took = false;
                    if (device_lock_acquire(dev, &took) != 0 || !took) errors += 1;
                    if (share_wants_staged(dev)) errors += 1;
                    if (took) device_lock_release(dev);
                }
                rounds += 1;
            }
        });
    for (std::thread& t : ts) t.join();
    EXPECT(errors.load() == 0 && rounds.load() == 1600);
    EXPECT(c.finish() == 0);
    EXPECT(lock_refs(DEV_A) == 0 && lock_refs(DEV_B) == 0);
    EXPECT(flock_free(d + "/gpu_0000_c1_00_0.lock") && flock_free(d + "/gpu_0000_05_00_0.lock"));
    const long long n = g_share.lock_acquisitions.load();
    EXPECT(n >= 2 && n <= 2000);                           // (a nested or concurrent acquire takes no flock of its own)
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: share_host_check MODE [SCRATCH_DIR]\n");
        return 2;
    }
    g_mode = argv[1];
    const std::string mode = argv[1], scratch = argc > 2 ? argv[2] : "";
    if (mode == "dir") mode_dir();
    else if (mode == "dir-symlink" || mode == "dir-file") mode_no_dir();
    else if (mode == "lock-symlink") mode_lock_symlink();
    else if (mode == "lock") mode_lock();
    else if (mode == "timeout") mode_timeout();
    else if (mode == "fork") mode_fork();
    else if (mode == "slots") mode_slots();
    else if (mode == "slots-off") mode_slots_off();
    else if (mode == "kfd" && !scratch.empty()) mode_kfd(scratch);
    else if (mode == "kfd-off" && !scratch.empty()) mode_kfd_off(scratch);
    else if (mode == "policy") mode_policy();
    else if (mode == "policy-nolock") mode_policy_nolock();
    else if (mode == "policy-dag") mode_policy_pinned(false);
    else if (mode == "policy-staged") mode_policy_pinned(true);
    else if (mode == "knobs") mode_knobs();
    else if (mode == "threads") mode_threads();
    else {
        fprintf(stderr, "share_host_check: unknown mode %s\n", argv[1]);
        return 2;
    }
    printf("%s ok\n", argv[1]);
    return 0;
}
