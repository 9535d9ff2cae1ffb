// shard_comm.hip — ONE config block built by the GPUs of a node, natively (SURVEY.md 8e level 2): the communicator and
// pag_shard_run, the whole sharded build behind one call.
//
// One process per GPU.  The two bulk exchanges — 12-byte tuples to their k-mer owners, and every rank's region of the
// finished graph from the owners (pag_shard_select) — are all-to-all(v)s of DEVICE buffers: RCCL over xGMI (grouped
// ncclSend / ncclRecv, the library loaded at run time), or, where RCCL cannot be used (two ranks on one device: the
// single-GPU test box), a transport through files of the rendezvous directory.  Small host-side tables (counts, sizes,
// statistics, the RCCL unique id, gathered travel sequences) always go through the rendezvous directory, which every rank of
// the node sees (/dev/shm by default): no second launcher, no sockets.
//
// Order argument for bit-identity with one GPU: see include/pagraph_hip.h (pag_shard_*) — rank r extracts the r-th contiguous
// range of the emission order, owners lay the received records out as [pass 1 from rank 0] .. [pass 1 from rank N-1]
// [pass 2 from rank 0] .. and sort stably by k-mer.  Where a record lies in that order is serial_layout.hpp's to say, not this file's.
#include <dirent.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <rccl/rccl.h>  // types and prototypes only: the entry points are resolved with dlsym (no link-time dependency)
#include <signal.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "dev_call.hpp"
#include "pag_graph_impl.hpp"
#include "serial_layout.hpp"

namespace {

// the few RCCL entry points used, with the signatures rccl.h declares them with (decltype of the prototypes), resolved
// with dlsym so that the library only depends on RCCL when it is asked for
struct Rccl {
    void *lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    bool load() {
        for (const char *name : {"librccl.so.1", "librccl.so"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (lib) break;
        }
        if (!lib) return false;
        auto sym = [&](const char *n) { return dlsym(lib, n); };
        GetUniqueId = (decltype(GetUniqueId))sym("ncclGetUniqueId");
        CommInitRank = (decltype(CommInitRank))sym("ncclCommInitRank");
        CommDestroy = (decltype(CommDestroy))sym("ncclCommDestroy");
        CommAbort = (decltype(CommAbort))sym("ncclCommAbort");
        GroupStart = (decltype(GroupStart))sym("ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))sym("ncclGroupEnd");
        Send = (decltype(Send))sym("ncclSend");
        Recv = (decltype(Recv))sym("ncclRecv");
        GetErrorString = (decltype(GetErrorString))sym("ncclGetErrorString");
        return GetUniqueId && CommInitRank && CommDestroy && GroupStart && GroupEnd && Send && Recv;
    }
};

using pagdev::now_s;

// start time of a process in clock ticks since boot (field 22 of /proc/<pid>/stat), 0 if it does not exist: (pid, start
// time) names ONE process for as long as the machine is up
unsigned long long proc_start(long pid) {
    char path[64];
    std::snprintf(path, sizeof path, "/proc/%ld/stat", pid);
    FILE *f = std::fopen(path, "r");
    if (!f) return 0;
    char buf[1024];
    const size_t n = std::fread(buf, 1, sizeof buf - 1, f);
    std::fclose(f);
    buf[n] = 0;
    const char *p = std::strrchr(buf, ')');  // (the command name may hold blanks and parentheses)
    if (!p) return 0;
    unsigned long long v = 0;
    int field = 2;
    for (++p; *p && field < 22;) {
        while (*p == ' ') ++p;
        ++field;
        if (field == 22) {
            v = std::strtoull(p, nullptr, 10);
            break;
        }
        while (*p && *p != ' ') ++p;
    }
    return v;
}

}  // namespace

struct pag_comm {
    int rank = 0, world = 1, device = 0;
    std::string dir;
    bool use_rccl = false;
    Rccl rccl;
    ncclComm_t comm = nullptr;
    hipStream_t stream = nullptr;
    uint64_t seq = 0;       // every collective of the job takes the next number (all ranks call them in the same order)
    double timeout_s = 600;
    uint64_t bytes_sent = 0;  // payload of the bulk exchanges that left this rank (wire volume)
    // Every file of the job carries the job's nonce in its name (agreed at creation, see handshake()): what an earlier
    // job — crashed, or still running in the same directory — left or leaves there is never read.
    unsigned long long job = 0;
    bool aborted = false;
    std::vector<std::pair<uint64_t, std::string>> kept;  // all-gather files of mine that peers may still read: (collective, path)

    std::string path(const char *tag, uint64_t n, int a, int b = -1) const {
        char buf[128];
        if (b >= 0) std::snprintf(buf, sizeof buf, "/j%016llx_%s%llu_%d_%d", job, tag, (unsigned long long)n, a, b);
        else std::snprintf(buf, sizeof buf, "/j%016llx_%s%llu_%d", job, tag, (unsigned long long)n, a);
        return dir + buf;
    }
    std::string abort_path(int r) const {
        char buf[64];
        std::snprintf(buf, sizeof buf, "/j%016llx_abort_%d", job, r);
        return dir + buf;
    }
    // a file that appears complete or not at all (written under another name, then renamed)
    int put_file(const std::string &p, const void *data, size_t bytes) const {
        char suffix[48];
        std::snprintf(suffix, sizeof suffix, ".part%d_%ld", rank, (long)getpid());
        const std::string tmp = p + suffix;
        FILE *f = std::fopen(tmp.c_str(), "wb");
        if (!f) {
            pagdev::set_error("pag_comm: cannot write %s", tmp.c_str());
            return PAG_EFAULT;
        }
        const bool ok = bytes == 0 || std::fwrite(data, 1, bytes, f) == bytes;
        if (std::fclose(f) != 0 || !ok || std::rename(tmp.c_str(), p.c_str()) != 0) {
            pagdev::set_error("pag_comm: cannot write %s", p.c_str());
            return PAG_EFAULT;
        }
        return PAG_OK;
    }
    static bool slurp(const std::string &p, std::vector<char> &out) {
        FILE *f = std::fopen(p.c_str(), "rb");
        if (!f) return false;
        out.clear();
        char buf[4096];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
        std::fclose(f);
        return true;
    }
    // a peer that failed says so (pag_comm_abort): the waiting ranks report ITS message at once instead of timing out
    bool peer_aborted() const {
        if (!job) return false;
        std::vector<char> msg;
        for (int r = 0; r < world; ++r) {
            if (r == rank) continue;
            struct stat st;
            const std::string ap = abort_path(r);
            if (stat(ap.c_str(), &st) != 0) continue;
            slurp(ap, msg);
            msg.push_back(0);
            pagdev::set_error("pag_comm: rank %d has failed: %s", r, msg.data());
            return true;
        }
        return false;
    }
    int get_file(const std::string &p, std::vector<char> &out, bool remove_after) const {
        const double t0 = now_s();
        struct stat st;
        for (unsigned spin = 0; stat(p.c_str(), &st) != 0; ++spin) {
            if ((spin & 63u) == 63u && peer_aborted()) return PAG_EFAULT;
            if (now_s() - t0 > timeout_s) {
                pagdev::set_error("pag_comm: rank %d waited %.0f s for %s (a peer has failed or never started)", rank, timeout_s, p.c_str());
                return PAG_EFAULT;
            }
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
        out.resize((size_t)st.st_size);
        FILE *f = std::fopen(p.c_str(), "rb");
        if (!f || (out.size() && std::fread(out.data(), 1, out.size(), f) != out.size())) {
            if (f) std::fclose(f);
            pagdev::set_error("pag_comm: cannot read %s", p.c_str());
            return PAG_EFAULT;
        }
        std::fclose(f);
        if (remove_after) std::remove(p.c_str());
        return PAG_OK;
    }
    // all-gather files of collectives before `done` have been read by every peer (each of them has since written a file
    // of a later collective, which it only does after leaving the earlier one)
    void drop_kept(uint64_t done) {
        size_t w = 0;
        for (size_t i = 0; i < kept.size(); ++i) {
            if (kept[i].first < done) std::remove(kept[i].second.c_str());
            else kept[w++] = kept[i];
        }
        kept.resize(w);
    }

    // The ranks of ONE job find each other in a directory that may hold the files of other jobs.  Every rank publishes
    // hello_<rank> = (pid, process start time, a random word); rank 0 waits until every rank's hello names a LIVE process
    // (what a crashed job left names a dead one and is ignored until its successor overwrites it), draws the job's nonce and
    // answers every rank with job_<rank> = (nonce, the random word it saw).  A rank takes the answer that echoes ITS word —
    // an answer left by an earlier job echoes another.  Two live jobs in one directory: the second hello of a rank
    // overwrites the first, one of the two jobs never gets its echo and times out with a message that says so.
    int handshake() {
        if (world == 1) {
            job = std::random_device{}() | ((unsigned long long)std::random_device{}() << 32) | 1ull;
            return PAG_OK;
        }
        struct Hello {
            long long pid;
            unsigned long long start, word;
        } me{(long long)getpid(), proc_start(getpid()), std::random_device{}() | ((unsigned long long)std::random_device{}() << 32)};
        struct Job {
            unsigned long long nonce, word;
        };
        char name[64];
        std::snprintf(name, sizeof name, "/hello_%d", rank);
        int rc = put_file(dir + name, &me, sizeof me);
        if (rc) return rc;
        const double t0 = now_s();
        std::vector<char> blob;
        if (rank == 0) {
            std::vector<Hello> seen(world);
            seen[0] = me;
            for (int r = 1; r < world; ++r) {
                std::snprintf(name, sizeof name, "/hello_%d", r);
                for (;;) {
                    Hello h{};
                    if (slurp(dir + name, blob) && blob.size() == sizeof h) {
                        std::memcpy(&h, blob.data(), sizeof h);
                        // (PAG_COMM_ANY_NAMESPACE=1: the ranks run in containers with PID namespaces of their own — one per GPU
                        // sharing the rendezvous directory — where /proc/<pid> of a peer is not this process's to see: a hello
                        // is then taken when the directory is the job's own fresh one, which is the launcher's to guarantee)
                        static const bool any_ns = pagdev::env_int("PAG_COMM_ANY_NAMESPACE", 0) != 0;
                        if (h.start != 0 && (any_ns || proc_start((long)h.pid) == h.start)) {
                            seen[r] = h;
                            break;
                        }
                    }
                    if (now_s() - t0 > timeout_s) {
                        pagdev::set_error("pag_comm_create: rank 0 waited %.0f s for a live rank %d in %s", timeout_s, r, dir.c_str());
                        return PAG_EFAULT;
                    }
                    std::this_thread::sleep_for(std::chrono::microseconds(500));
                }
            }
            job = std::random_device{}() | ((unsigned long long)std::random_device{}() << 32) | 1ull;
            for (int r = 1; r < world; ++r) {
                Job j{job, seen[r].word};
                std::snprintf(name, sizeof name, "/job_%d", r);
                if ((rc = put_file(dir + name, &j, sizeof j))) return rc;
            }
            return PAG_OK;
        }
        std::snprintf(name, sizeof name, "/job_%d", rank);
        for (;;) {
            Job j{};
            if (slurp(dir + name, blob) && blob.size() == sizeof j) {
                std::memcpy(&j, blob.data(), sizeof j);
                if (j.word == me.word) {
                    job = j.nonce;
                    std::remove((dir + name).c_str());
                    return PAG_OK;
                }
            }
            if (now_s() - t0 > timeout_s) {
                pagdev::set_error("pag_comm_create: rank %d waited %.0f s for rank 0's answer in %s (no rank 0, or another job is using the directory)",
                                  rank, timeout_s, dir.c_str());
                return PAG_EFAULT;
            }
            std::this_thread::sleep_for(std::chrono::microseconds(500));
        }
    }
};

extern "C" {

pag_comm *pag_comm_create(int rank, int world, const char *rendezvous_dir, int device, const char *transport, int *err) {
    auto fail = [&](int code) -> pag_comm * {
        if (err) *err = code;
        return nullptr;
    };
    if (rank < 0 || world < 1 || rank >= world || !rendezvous_dir) return fail(PAG_EINVAL);
    pag_comm *c = new pag_comm();
    c->rank = rank;
    c->world = world;
    c->device = device;
    c->dir = rendezvous_dir;
    if (const char *e = std::getenv("PAG_COMM_TIMEOUT_S")) c->timeout_s = std::max(1.0, std::atof(e));
    mkdir(c->dir.c_str(), 0700);  // (every rank tries; the directory may exist)
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        pagdev::set_error("pag_comm_create: device %d unusable", device);
        delete c;
        return fail(PAG_ENODEV);
    }
    if (c->handshake() != PAG_OK) {
        hipStreamDestroy(c->stream);
        delete c;
        return fail(PAG_EFAULT);
    }
    const bool want_rccl = !transport || std::strcmp(transport, "rccl") == 0;
    // (PAG_COMM_FORCE_RCCL=1: also for a world of one — exercises the RCCL calls on a single-GPU box)
    if (want_rccl && (world > 1 || (std::getenv("PAG_COMM_FORCE_RCCL") && transport && std::strcmp(transport, "rccl") == 0))) {
        if (!c->rccl.load()) {
            pagdev::set_error("pag_comm_create: librccl.so not found (transport \"host\" goes through the rendezvous directory)");
            pag_comm_destroy(c);
            return fail(PAG_ENODEV);
        }
        ncclUniqueId id{};
        std::vector<char> blob;
        int rc = PAG_OK;
        const std::string idp = c->path("rcclid", 0, 0);
        if (rank == 0) {
            if (c->rccl.GetUniqueId(&id) != ncclSuccess) rc = PAG_EFAULT;
            else rc = c->put_file(idp, &id, sizeof id);
        } else {
            rc = c->get_file(idp, blob, false);
            if (rc == PAG_OK && blob.size() == sizeof id) std::memcpy(&id, blob.data(), sizeof id);
            else if (rc == PAG_OK) rc = PAG_EFAULT;
        }
        const ncclResult_t nrc = rc == PAG_OK ? c->rccl.CommInitRank(&c->comm, world, id, rank) : ncclSystemError;
        if (rank == 0 && rc == PAG_OK) c->kept.push_back({0, idp});  // (read by every peer before its CommInitRank returns)
        if (rc != PAG_OK || nrc != ncclSuccess) {
            pagdev::set_error("pag_comm_create: RCCL communicator of %d ranks failed (%s)", world,
                              rc == PAG_OK && c->rccl.GetErrorString ? c->rccl.GetErrorString(nrc) : "rendezvous");
            c->comm = nullptr;
            pag_comm_destroy(c);
            return fail(PAG_EFAULT);
        }
        c->use_rccl = true;
    }
    if (err) *err = PAG_OK;
    return c;
}

void pag_comm_destroy(pag_comm *c) {
    if (!c) return;
    if (c->comm) {
        // a communicator whose job failed may have peers that never arrive: abort instead of the collective destroy
        if (c->aborted && c->rccl.CommAbort) c->rccl.CommAbort(c->comm);
        else c->rccl.CommDestroy(c->comm);
    }
    if (c->stream) hipStreamDestroy(c->stream);
    // (the files of this rank's LAST all-gather may still be read by a peer; whatever stays carries the job's nonce and is
    // never taken for another job's)
    if (!c->kept.empty()) c->drop_kept(c->kept.back().first);
    char name[64];
    std::snprintf(name, sizeof name, "/hello_%d", c->rank);
    std::remove((c->dir + name).c_str());
    delete c;
}
int pag_comm_rank(const pag_comm *c) { return c ? c->rank : -1; }
int pag_comm_world(const pag_comm *c) { return c ? c->world : 0; }
uint64_t pag_comm_bytes_sent(const pag_comm *c) { return c ? c->bytes_sent : 0; }

// This rank cannot go on (message: why): every peer that waits for it — now or later — fails at once with that message
// instead of waiting for its timeout.
void pag_comm_abort(pag_comm *c, const char *message) {
    if (!c || c->aborted) return;
    c->aborted = true;
    if (c->world == 1 || !c->job) return;
    const char *m = message && *message ? message : "(no message)";
    const std::string keep(m);  // (put_file may overwrite the error buffer `message` points into)
    c->put_file(c->abort_path(c->rank), keep.data(), keep.size());
}

// every rank contributes `bytes` of host memory; all[r * bytes ..] = rank r's
int pag_comm_all_gather(pag_comm *c, const void *mine, uint64_t bytes, void *all) {
    if (!c || (!mine && bytes) || !all) return PAG_EINVAL;
    const uint64_t n = c->seq++;
    if (c->world == 1) {
        std::memcpy(all, mine, bytes);
        return PAG_OK;
    }
    if (c->aborted) {
        pagdev::set_error("pag_comm: this rank has aborted the job");
        return PAG_EFAULT;
    }
    const std::string minep = c->path("g", n, c->rank);
    int rc = c->put_file(minep, mine, bytes);
    if (rc) return rc;
    c->kept.push_back({n, minep});
    std::vector<char> blob;
    for (int r = 0; r < c->world; ++r) {
        if ((rc = c->get_file(c->path("g", n, r), blob, false))) return rc;
        if (blob.size() != bytes) {
            pagdev::set_error("pag_comm_all_gather: rank %d sent %zu bytes, %llu expected", r, blob.size(), (unsigned long long)bytes);
            return PAG_EFAULT;
        }
        std::memcpy((char *)all + (size_t)r * bytes, blob.data(), bytes);
    }
    c->drop_kept(n);  // every peer has written its file of collective n: it has left every earlier collective
    return PAG_OK;
}
int pag_comm_barrier(pag_comm *c) {
    char x = 0;
    std::vector<char> all(c ? (size_t)c->world : 1);
    return pag_comm_all_gather(c, &x, 1, all.data());
}
// host blobs of any size to `root`: sizes[r] / offsets into `out` (capacity out_cap, required size returned in *need)
int pag_comm_gather_v(pag_comm *c, const void *mine, uint64_t bytes, int root, void *out, uint64_t out_cap, uint64_t *sizes, uint64_t *need) {
    if (!c || (!mine && bytes)) return PAG_EINVAL;
    const uint64_t n = c->seq++;
    int rc;
    if (c->rank != root) return c->put_file(c->path("v", n, c->rank), mine, bytes);
    uint64_t at = 0;
    std::vector<char> blob;
    for (int r = 0; r < c->world; ++r) {
        const void *src = mine;
        uint64_t sz = bytes;
        if (r != root) {
            if ((rc = c->get_file(c->path("v", n, r), blob, true))) return rc;
            src = blob.data();
            sz = blob.size();
        }
        if (sizes) sizes[r] = sz;
        if (out && at + sz <= out_cap && sz) std::memcpy((char *)out + at, src, sz);
        at += sz;
    }
    if (need) *need = at;
    return at <= out_cap ? PAG_OK : PAG_ERANGE;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// The bulk exchange: several device arrays, each an all-to-all(v) — sb[d] consecutive bytes of `send` go to rank d, rb[s] bytes
// arrive from rank s, in rank order on both sides.  It runs IN THE BACKGROUND (round 5), begun by xchg_begin and waited for by
// xchg_end, so that the next piece of work of the call's own stream — the next chunk's extraction, the next destination's
// selection — runs beside it.  RCCL: the grouped sends / receives of all arrays are enqueued on the communicator's stream (a
// stream of its own, non-blocking) and xchg_end waits for that stream.  Files of the rendezvous directory (ranks that share a
// device: the single-GPU test boxes): a helper thread passes them, with copies on the communicator's stream.  One exchange at a
// time per communicator.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
struct Xchg {
    pag_comm *c = nullptr;
    bool active = false;
    std::thread th;
    int rc = PAG_OK;
    std::string err;
    double t_begin = 0, t_done = 0;  // (host clock; t_done is set when the transfer is known to be over)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float dev_ms = 0.f;
};
struct XchgArr {
    const void *send;
    void *recv;
    std::vector<uint64_t> sb, rb;  // bytes to / from every rank
};

int xchg_files(pag_comm *c, uint64_t n, const XchgArr &A, std::string &err) {
    std::vector<uint64_t> so(c->world + 1, 0), ro(c->world + 1, 0);
    for (int r = 0; r < c->world; ++r) {
        so[r + 1] = so[r] + A.sb[r];
        ro[r + 1] = ro[r] + A.rb[r];
    }
    auto hip_ok = [&](hipError_t e, const char *what) {
        if (e == hipSuccess) return true;
        err = std::string(what) + ": " + hipGetErrorString(e);
        return false;
    };
    std::vector<char> host;
    int rc;
    for (int d = 0; d < c->world; ++d) {
        if (d == c->rank) continue;
        host.resize(A.sb[d]);
        if (A.sb[d] && !(hip_ok(hipMemcpyAsync(host.data(), (const char *)A.send + so[d], A.sb[d], hipMemcpyDeviceToHost, c->stream), "copy to host") &&
                         hip_ok(hipStreamSynchronize(c->stream), "copy to host")))
            return PAG_EFAULT;
        if ((rc = c->put_file(c->path("a", n, c->rank, d), host.data(), A.sb[d]))) {
            err = pagdev::last_error();
            return rc;
        }
    }
    if (A.sb[c->rank] && !(hip_ok(hipMemcpyAsync((char *)A.recv + ro[c->rank], (const char *)A.send + so[c->rank], A.sb[c->rank], hipMemcpyDeviceToDevice, c->stream), "own part") &&
                           hip_ok(hipStreamSynchronize(c->stream), "own part")))
        return PAG_EFAULT;
    for (int s2 = 0; s2 < c->world; ++s2) {
        if (s2 == c->rank) continue;
        if ((rc = c->get_file(c->path("a", n, s2, c->rank), host, true))) {
            err = pagdev::last_error();
            return rc;
        }
        if (host.size() != A.rb[s2]) {
            err = "exchange: " + std::to_string(host.size()) + " bytes from rank " + std::to_string(s2) + ", " + std::to_string(A.rb[s2]) + " expected";
            return PAG_EFAULT;
        }
        if (A.rb[s2] && !(hip_ok(hipMemcpyAsync((char *)A.recv + ro[s2], host.data(), A.rb[s2], hipMemcpyHostToDevice, c->stream), "copy to device") &&
                          hip_ok(hipStreamSynchronize(c->stream), "copy to device")))
            return PAG_EFAULT;
    }
    return PAG_OK;
}

// (the caller's data — send arrays written on another stream — must be complete: the caller synchronises its stream first)
int xchg_begin(pag_comm *c, Xchg &X, std::vector<XchgArr> arrs) {
    X.c = c;
    X.rc = PAG_OK;
    X.err.clear();
    X.dev_ms = 0.f;
    PAG_HIP_TRY(hipSetDevice(c->device));
    for (const XchgArr &A : arrs) {
        if (A.sb[c->rank] != A.rb[c->rank]) return PAG_EINVAL;
        for (int r = 0; r < c->world; ++r)
            if (r != c->rank) c->bytes_sent += A.sb[r];
    }
    X.t_begin = now_s();
    if (c->use_rccl) {
        // a grouped Send / Recv whose peer never arrives waits for ever: the ranks first meet through the rendezvous directory
        // (where a failed peer's abort marker is seen), and only a complete set of ranks enters RCCL
        if (c->world > 1) {
            const int brc = pag_comm_barrier(c);
            if (brc) return brc;
        }
        if (!X.ev0) {
            PAG_HIP_TRY(hipEventCreate(&X.ev0));
            PAG_HIP_TRY(hipEventCreate(&X.ev1));
        }
        PAG_HIP_TRY(hipEventRecord(X.ev0, c->stream));
        ncclResult_t rc = c->rccl.GroupStart();
        for (const XchgArr &A : arrs) {
            uint64_t so = 0, ro = 0;
            for (int r = 0; r < c->world && rc == ncclSuccess; ++r) {
                if (A.sb[r]) rc = c->rccl.Send((const char *)A.send + so, A.sb[r], ncclUint8, r, c->comm, c->stream);
                if (rc == ncclSuccess && A.rb[r]) rc = c->rccl.Recv((char *)A.recv + ro, A.rb[r], ncclUint8, r, c->comm, c->stream);
                so += A.sb[r];
                ro += A.rb[r];
            }
        }
        const ncclResult_t rc2 = c->rccl.GroupEnd();
        if (rc != ncclSuccess || rc2 != ncclSuccess) {
            pagdev::set_error("exchange: RCCL error %s", c->rccl.GetErrorString ? c->rccl.GetErrorString(rc != ncclSuccess ? rc : rc2) : "?");
            return PAG_EFAULT;
        }
        PAG_HIP_TRY(hipEventRecord(X.ev1, c->stream));
        X.active = true;
        return PAG_OK;
    }
    std::vector<uint64_t> seqs;
    for (size_t a = 0; a < arrs.size(); ++a) seqs.push_back(c->seq++);
    try {
        X.th = std::thread([c, &X, arrs = std::move(arrs), seqs]() {
            if (hipSetDevice(c->device) != hipSuccess) {
                X.rc = PAG_EFAULT;
                X.err = "hipSetDevice in the exchange thread";
            }
            for (size_t a = 0; a < arrs.size() && X.rc == PAG_OK; ++a) X.rc = xchg_files(c, seqs[a], arrs[a], X.err);
            X.t_done = now_s();
        });
    } catch (const std::exception &e) {  // (no thread to be had: nothing was started)
        pagdev::set_error("exchange: cannot start the helper thread: %s", e.what());
        return PAG_EFAULT;
    }
    X.active = true;
    return PAG_OK;
}
int xchg_end(Xchg &X) {
    if (!X.active) return PAG_OK;
    X.active = false;
    if (X.c->use_rccl) {
        PAG_HIP_TRY(hipStreamSynchronize(X.c->stream));
        PAG_HIP_TRY(hipEventElapsedTime(&X.dev_ms, X.ev0, X.ev1));
        X.t_done = X.t_begin + X.dev_ms * 1e-3;
        return PAG_OK;
    }
    X.th.join();
    if (X.rc != PAG_OK) pagdev::set_error("%s", X.err.c_str());
    return X.rc;
}
struct XchgGuard {  // (an error return between begin and end must not leave a joinable thread behind)
    Xchg &X;
    ~XchgGuard() {
        if (X.active && !X.c->use_rccl && X.th.joinable()) X.th.join();
        // (RCCL: the grouped sends / receives of an exchange that was begun and never ended read and write the chunk buffers the
        // caller is about to free — they are waited for first; a peer that has died makes this wait end with the communicator's
        // own error, which the caller is returning anyway)
        if (X.active && X.c->use_rccl) (void)hipStreamSynchronize(X.c->stream);
        if (X.ev0) hipEventDestroy(X.ev0);
        if (X.ev1) hipEventDestroy(X.ev1);
    }
};
}  // namespace

// all-to-all(v) of DEVICE memory, one array, waited for: the exchange above, begun and ended
extern "C" int pag_comm_all_to_all_v(pag_comm *c, const void *send, const uint64_t *send_bytes, void *recv, const uint64_t *recv_bytes) {
    if (!c || !send_bytes || !recv_bytes) return PAG_EINVAL;
    PAG_HIP_TRY(hipSetDevice(c->device));
    // The exchange works on the communicator's own stream, which is ordered behind no other: what the caller queued on the device
    // before this call — the null stream's work included — is waited for here, so that `send` holds what the caller put there.
    PAG_HIP_TRY(hipDeviceSynchronize());
    Xchg X;
    XchgGuard guard{X};
    const int rc = xchg_begin(c, X, {XchgArr{send, recv, {send_bytes, send_bytes + c->world}, {recv_bytes, recv_bytes + c->world}}});
    return rc ? rc : xchg_end(X);
}

// ---------------------------------------------------------------------------------------------------------------------
// pag_shard_run: the sharded build of one block behind one call (every rank calls it with the same prepared input).  Its stages:
//   1. exchange_streams        own read range extracted in chunks, every chunk's tuple / edge streams to their owners
//   2. lay_out_owned           what arrived, in the owner's canonical order (the plan of serial_layout.hpp)
//   3. build_owned             K2-K4 on the owned k-mer range
//   4. exchange_regions_ring   every rank's region selected from the slice and sent to it, a selection beside the next one
//      / exchange_regions_whole  (PAG_SHARD_PIPELINE=0) all selections first, then seven whole all-to-all(v)s
//   5. adopt_region            what arrived becomes the handle's graph, region set, the build's memory released
// regions[world]: what every rank traverses (the same on all ranks); total: the block's count lines.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
using namespace pagdev;

// PAGRAPH_TIMING=1: one line per rank and block on stderr — seconds per stage of this call (the device idle at every boundary)
// and the payload that left the rank in each of the two bulk exchanges.  Without it the clock neither synchronises nor counts.
struct StageClock {
    const bool on = env_timing();
    double t_prev = now();
    double now() const {
        if (on) hipDeviceSynchronize();
        return now_s();
    }
    double lap() {  // seconds since the lap before
        if (!on) return 0;
        const double t = now(), d = t - t_prev;
        t_prev = t;
        return d;
    }
};

// The books of a loop whose step i runs beside the exchange begun after step i - 1 (host clock): seconds of the steps, of the
// exchanges, of the exchanges that passed beside a step, and of the whole loop; [step0, step1]: the step that ended last.
struct OverlapBooks {
    double step = 0, xfer = 0, hidden = 0, loop = 0;
    double t_loop = 0, step0 = 0, step1 = 0;
};
// the exchange under way, if there is one, is waited for and booked; beside_step: it travelled beside the step that has just ended
int xchg_end_booked(Xchg &X, OverlapBooks &B, bool beside_step) {
    const bool was_active = X.active;
    const int rc = xchg_end(X);
    if (rc || !was_active) return rc;
    B.xfer += X.t_done - X.t_begin;
    if (beside_step) B.hidden += std::max(0.0, std::min(X.t_done, B.step1) - std::max(X.t_begin, B.step0));
    return PAG_OK;
}

constexpr int NA = ps::GRAPH_ARRS, NT = ps::GRAPH_TUPLE_ARRS;  // the seven arrays of a graph, the first four per tuple
ps::Id send_slot(int a) { return ps::family(ps::SEND, a); }    // the send buffers of the region exchange

struct ShardRun {
    pag_graph *g;
    pag_comm *c;
    const pag_build_input *in;
    const pag_region *regions;
    const int W, me;
    hipStream_t s;
    StageClock clock;
    // 1 -> 2: counts[chunk_range(rank, C, chunk)][owner][4] (serial_layout.hpp), the chunks' arrays (tkey tval ekey eval each)
    int C = 4;
    std::vector<uint64_t> counts;
    struct ChunkBufs {
        void *send[4] = {}, *recv[4] = {};  // this rank's chunk, partitioned by owner; what the ranks sent of theirs
    };
    std::vector<ChunkBufs> cb;
    DevCall tmp{"pag_shard_run"}, sent{"pag_shard_run"};  // the chunks as received; this rank's copies of them on their way out
    // 2 -> 3: the owner's streams and the plan they were laid out by, its sizes with it ([0] tuples, [1] edges)
    DevBuf own[4];
    ReceivePlan plan[2];
    // 4 -> 5: the region in the import slots, the statistics of what owner o selected for this rank
    uint64_t T = 0, E = 0;
    std::vector<pag_build_stats> from_owner = std::vector<pag_build_stats>((size_t)W);
    // the [shard timing] line
    OverlapBooks tuple_books, region_books;
    double s_layout = 0, s_build = 0, s_owner_order = 0, s_adopt = 0;
};

// 1. Extraction in CHUNKS, every chunk's partitioned streams on their way to the owners while the next chunk is extracted
//    (SURVEY.md 8e).  PAG_SHARD_CHUNKS (default 4; 1: the whole range at once).  A chunk's streams are copied out of the
//    extraction's slots (the next chunk overwrites them) and received into arrays of their own.
int exchange_streams(ShardRun &R) {
    pag_graph *g = R.g;
    const int W = R.W, me = R.me, C = R.C;
    int rc;
    const uint64_t n_reads = R.in->reads.n_seqs, r_lo = n_reads * (uint64_t)me / (uint64_t)W, r_hi = n_reads * ((uint64_t)me + 1) / (uint64_t)W;
    R.counts.assign((size_t)W * C * W * 4, 0);
    R.cb.resize((size_t)C);
    std::vector<uint64_t> mine(4 * (size_t)W), all(4 * (size_t)W * W);
    Xchg X;
    XchgGuard xguard{X};
    OverlapBooks &B = R.tuple_books;
    B.t_loop = now_s();
    for (int ch = 0; ch < C; ++ch) {
        const uint64_t lo = r_lo + (r_hi - r_lo) * (uint64_t)ch / (uint64_t)C, hi = r_lo + (r_hi - r_lo) * ((uint64_t)ch + 1) / (uint64_t)C;
        ShardRun::ChunkBufs &cb = R.cb[(size_t)ch];
        B.step0 = now_s();
        if ((rc = pag_shard_extract_range(g, R.in, lo, hi, (uint32_t)W, mine.data()))) return rc;
        for (int a = 0; a < 4; ++a) {
            char *q = nullptr;
            if ((rc = R.sent.alloc(&q, (g->shard_x[a / 2] + 1) * ps::STREAM_ESZ[a]))) return rc;
            cb.send[a] = q;
        }
        const StreamPtrs part = streams_at(g, g->shard_in0[0], g->shard_in0[1]);
        if ((rc = copy_streams(part, 0, g->shard_x[0], 0, g->shard_x[1], cb.send[0], cb.send[1], cb.send[2], cb.send[3], R.s))) return rc;
        PAG_HIP_TRY(hipStreamSynchronize(R.s));
        B.step += (B.step1 = now_s()) - B.step0;
        if ((rc = pag_comm_all_gather(R.c, mine.data(), mine.size() * 8, all.data()))) return rc;
        for (int r = 0; r < W; ++r)
            std::memcpy(&R.counts[(size_t)chunk_range(r, C, ch) * W * 4], &all[(size_t)r * W * 4], (size_t)W * 4 * 8);
        // the chunk before this one has been travelling beside this extraction
        if ((rc = xchg_end_booked(X, B, true))) return rc;
        std::vector<XchgArr> arrs(4);
        for (int a = 0; a < 4; ++a) {
            uint64_t tot = 0;
            arrs[a].sb.resize(W);
            arrs[a].rb.resize(W);
            for (int r = 0; r < W; ++r) {
                arrs[a].sb[r] = range_records(R.counts.data(), W, chunk_range(me, C, ch), r, a / 2) * ps::STREAM_ESZ[a];
                arrs[a].rb[r] = range_records(R.counts.data(), W, chunk_range(r, C, ch), me, a / 2) * ps::STREAM_ESZ[a];
                tot += arrs[a].rb[r];
            }
            char *q = nullptr;
            if ((rc = R.tmp.alloc(&q, tot + ps::STREAM_ESZ[a]))) return rc;
            arrs[a].send = cb.send[a];
            arrs[a].recv = cb.recv[a] = q;
        }
        if ((rc = xchg_begin(R.c, X, std::move(arrs)))) return rc;
    }
    if ((rc = xchg_end_booked(X, B, false))) return rc;
    B.loop = now_s() - B.t_loop;
    return PAG_OK;
}

// 2. When the last chunk has arrived the owner lays the pieces out as [pass 1: rank 0 chunk 0, chunk 1 .. rank 1 ..][pass 2: ..] —
//    the ranks' read ranges and, inside a rank, its chunks are contiguous in emission order, so that is the canonical order
//    again.  chunked_receive_plan knows where everything lies; here its copies are made.
int lay_out_owned(ShardRun &R) {
    int rc;
    R.sent.release();  // (the chunks' send copies are done with)
    for (int st = 0; st < 2; ++st) R.plan[st] = chunked_receive_plan(R.counts.data(), R.W, R.C, R.me, st);
    const ps::Id slot[4] = {ps::OWN_TK, ps::OWN_TV, ps::OWN_EK, ps::OWN_EV};
    for (int a = 0; a < 4; ++a) {
        R.own[a] = DevBuf(R.g, slot[a]);
        if ((rc = R.own[a].alloc((R.plan[a / 2].n + 1) * ps::STREAM_ESZ[a]))) return rc;
    }
    for (int a = 0; a < 4; ++a) {
        const uint64_t esz = ps::STREAM_ESZ[a];
        for (const ReceivePlan::Copy &cp : R.plan[a / 2].copies)
            PAG_HIP_TRY(hipMemcpyAsync((char *)R.own[a].p + cp.dst * esz, (const char *)R.cb[cp.chunk].recv[a] + cp.src * esz, cp.n * esz, hipMemcpyDeviceToDevice, R.s));
    }
    PAG_HIP_TRY(hipStreamSynchronize(R.s));
    R.tmp.release();
    return PAG_OK;
}

// 3. K2-K4 on what this owner holds
int build_owned(ShardRun &R) {
    pag_build_stats mine{};
    return pag_shard_build(R.g, R.own[0].as<uint32_t>(), R.own[1].as<uint64_t>(), R.plan[0].n, R.plan[0].n1, R.own[2].as<uint32_t>(), R.own[3].as<uint64_t>(),
                           R.plan[1].n, R.plan[1].n1, R.in->eps, &mine);
}

// 4. Every rank's region of this owner's slice.  A selection lives in the handle until the next one: it is copied behind the
//    previous ones into the send buffers, which are sized once for what the selections of all destinations usually add up to — the
//    slice itself plus the landing zones and halos that several ranks take (1.2x at N = 4, measured) — so that the loops below
//    neither allocate nor copy what they have already gathered; a block that needs more grows them.
int reserve_send_buffers(ShardRun &R) {
    int rc;
    for (int a = 0; a < NA; ++a) {
        const uint64_t n_slice = a < NT ? R.g->n_t : R.g->n_e;
        if ((rc = DevBuf(R.g, send_slot(a)).alloc((n_slice + n_slice / 2 + 1024) * ps::GRAPH_ESZ[a]))) return rc;
    }
    return PAG_OK;
}
// the selection `sel` behind the at[a] elements array a of the send buffers holds (at: advanced).  A buffer that is too small is
// grown with its contents kept; X: an exchange that may still read the old array and is waited for first (null: there is none)
int append_selection(ShardRun &R, const pag_shard_slice &sel, std::vector<uint64_t> &at, Xchg *X) {
    int rc;
    const GraphArrays from = arrays_of(sel);
    for (int a = 0; a < NA; ++a) {
        const uint64_t n = a < NT ? sel.n_t : sel.n_e, esz = ps::GRAPH_ESZ[a], need = (at[a] + n + 1) * esz;
        DevBuf b(R.g, send_slot(a));
        if (b.sl->cap < need && ((X && (rc = xchg_end(*X))) || (rc = b.alloc_keeping(need, at[a] * esz, need + need / 2 + 256)))) return rc;
        if (n) PAG_HIP_TRY(hipMemcpyAsync((char *)b.sl->p + at[a] * esz, from.p[a], n * esz, hipMemcpyDeviceToDevice, R.s));
        at[a] += n;
    }
    PAG_HIP_TRY(hipStreamSynchronize(R.s));
    return PAG_OK;
}

// Ring schedule.  Step i: this owner selects the region of rank (me + i) mod W and receives, from rank (me - i) mod W, that
// owner's selection for this rank; the selection of step i travels while the one of step i + 1 is made.  What arrives is kept
// per owner and put in owner order (ascending k-mer ranges) when the last piece is there.
int exchange_regions_ring(ShardRun &R) {
    pag_graph *g = R.g;
    const int W = R.W, me = R.me;
    int rc;
    struct StepMsg {  // what an owner selected in this step: its size and count lines
        uint64_t n_t, n_e;
        pag_build_stats st;
    };
    std::vector<std::vector<void *>> piece((size_t)W, std::vector<void *>(NA, nullptr));  // [owner][array]
    std::vector<uint64_t> piece_t(W, 0), piece_e(W, 0), at(NA, 0);
    DevCall rtmp("pag_shard_run");
    Xchg X;
    XchgGuard xguard{X};
    OverlapBooks &B = R.region_books;
    B.t_loop = now_s();
    for (int i = 0; i < W; ++i) {
        const int dst = (me + i) % W, src = (me - i + W) % W;
        B.step0 = now_s();
        pag_shard_slice sel{};
        if ((rc = pag_shard_select(g, &R.regions[dst], &sel))) return rc;
        const std::vector<uint64_t> at0 = at;
        if ((rc = append_selection(R, sel, at, &X))) return rc;
        B.step += (B.step1 = now_s()) - B.step0;
        std::vector<StepMsg> msg(W);
        StepMsg mine_msg{sel.n_t, sel.n_e, sel.stats};
        if ((rc = pag_comm_all_gather(R.c, &mine_msg, sizeof mine_msg, msg.data()))) return rc;
        if ((rc = xchg_end_booked(X, B, true))) return rc;
        R.T += piece_t[(size_t)src] = msg[(size_t)src].n_t;  // (every owner is `src` in exactly one step)
        R.E += piece_e[(size_t)src] = msg[(size_t)src].n_e;
        R.from_owner[(size_t)src] = msg[(size_t)src].st;
        if (i == 0) continue;  // this rank's own selection stays where it is: at the front of the send buffers
        std::vector<XchgArr> xa(NA);
        for (int a = 0; a < NA; ++a) {
            const uint64_t n_out = a < NT ? sel.n_t : sel.n_e, n_in = a < NT ? piece_t[(size_t)src] : piece_e[(size_t)src], esz = ps::GRAPH_ESZ[a];
            char *q = nullptr;
            if ((rc = rtmp.alloc(&q, (n_in + 1) * esz))) return rc;
            piece[(size_t)src][a] = q;
            xa[a].sb.assign(W, 0);
            xa[a].rb.assign(W, 0);
            xa[a].sb[(size_t)dst] = n_out * esz;
            xa[a].rb[(size_t)src] = n_in * esz;
            xa[a].send = (const char *)g->pool[send_slot(a)].p + at0[a] * esz;
            xa[a].recv = q;
        }
        if ((rc = xchg_begin(R.c, X, std::move(xa)))) return rc;
    }
    if ((rc = xchg_end_booked(X, B, false))) return rc;
    B.loop = now_s() - B.t_loop;
    R.clock.lap();
    for (int a = 0; a < NA; ++a) {
        const uint64_t esz = ps::GRAPH_ESZ[a];
        DevBuf imp(g, ps::family(ps::IMPORT, a));
        if ((rc = imp.alloc(((a < NT ? R.T : R.E) + 1) * esz))) return rc;
        piece[(size_t)me][a] = g->pool[send_slot(a)].p;  // (where the send buffer is NOW: one that grew has moved)
        uint64_t off = 0;
        for (int o = 0; o < W; ++o) {  // owner order = ascending k-mer ranges
            const uint64_t n = a < NT ? piece_t[(size_t)o] : piece_e[(size_t)o];
            if (n) PAG_HIP_TRY(hipMemcpyAsync((char *)imp.p + off * esz, piece[(size_t)o][a], n * esz, hipMemcpyDeviceToDevice, R.s));
            off += n;
        }
    }
    PAG_HIP_TRY(hipStreamSynchronize(R.s));
    rtmp.release();
    R.s_owner_order = R.clock.lap();
    return PAG_OK;
}

// Whole schedule (PAG_SHARD_PIPELINE=0, as until round 5): all selections first, then seven whole all-to-all(v)s, received
// straight into the import slots — rank order there is owner order, ascending k-mer ranges
int exchange_regions_whole(ShardRun &R) {
    pag_graph *g = R.g;
    const int W = R.W, me = R.me;
    int rc;
    std::vector<uint64_t> my_sizes(2 * (size_t)W), all_sizes(2 * (size_t)W * W), at(NA, 0);
    std::vector<pag_build_stats> stats_to(W), all_stats((size_t)W * W);
    for (int d = 0; d < W; ++d) {
        pag_shard_slice sel{};
        if ((rc = pag_shard_select(g, &R.regions[d], &sel))) return rc;
        my_sizes[2 * d] = sel.n_t;
        my_sizes[2 * d + 1] = sel.n_e;
        stats_to[d] = sel.stats;
        if ((rc = append_selection(R, sel, at, nullptr))) return rc;
    }
    R.region_books.step = R.clock.lap();
    if ((rc = pag_comm_all_gather(R.c, my_sizes.data(), my_sizes.size() * 8, all_sizes.data()))) return rc;
    if ((rc = pag_comm_all_gather(R.c, stats_to.data(), stats_to.size() * sizeof(pag_build_stats), all_stats.data()))) return rc;
    auto size_of = [&](int owner, int dst, int which) { return all_sizes[((size_t)owner * W + dst) * 2 + which]; };
    for (int o = 0; o < W; ++o) {
        R.T += size_of(o, me, 0);
        R.E += size_of(o, me, 1);
        R.from_owner[(size_t)o] = all_stats[(size_t)o * W + me];
    }
    for (int a = 0; a < NA; ++a) {
        const uint64_t esz = ps::GRAPH_ESZ[a];
        DevBuf imp(g, ps::family(ps::IMPORT, a));
        if ((rc = imp.alloc(((a < NT ? R.T : R.E) + 1) * esz))) return rc;
        std::vector<uint64_t> sb(W), rb(W);
        for (int r = 0; r < W; ++r) {
            sb[r] = size_of(me, r, a < NT ? 0 : 1) * esz;
            rb[r] = size_of(r, me, a < NT ? 0 : 1) * esz;
        }
        if ((rc = pag_comm_all_to_all_v(R.c, g->pool[send_slot(a)].p, sb.data(), imp.p, rb.data()))) return rc;
    }
    R.region_books.xfer = R.clock.lap();
    return PAG_OK;
}

// 5. the graph arrays are in the import slots: the handle takes them over with the sums of the owners' statistics
int adopt_region(ShardRun &R, pag_build_stats *total) {
    int rc;
    pag_build_stats st{};
    for (const pag_build_stats &p : R.from_owner) add_stats(st, p);
    if ((rc = pag_shard_adopt(R.g, R.T, R.E, &st)) || (rc = pag_shard_set_region(R.g, &R.regions[R.me])) || (rc = pag_shard_release_build(R.g))) return rc;
    if (total) *total = st;
    return PAG_OK;
}

int shard_run(pag_graph *g, pag_comm *c, const pag_build_input *in, const pag_region *regions, pag_build_stats *total) {
    ShardRun R{g, c, in, regions, c->world, c->rank, g->stream};
    if (const char *e = std::getenv("PAG_SHARD_CHUNKS")) R.C = std::max(1, std::min(64, std::atoi(e)));
    const bool pipeline = env_int("PAG_SHARD_PIPELINE", 1) != 0;
    int rc;
    uint64_t wire[2];  // payload out in the two bulk exchanges
    const uint64_t sent0 = pag_comm_bytes_sent(c);
    if ((rc = exchange_streams(R))) return rc;
    wire[0] = pag_comm_bytes_sent(c) - sent0;
    R.clock.lap();
    if ((rc = lay_out_owned(R))) return rc;
    R.s_layout = R.clock.lap();
    if ((rc = build_owned(R))) return rc;
    R.s_build = R.clock.lap();
    if ((rc = reserve_send_buffers(R)) || (rc = pipeline ? exchange_regions_ring(R) : exchange_regions_whole(R))) return rc;
    wire[1] = pag_comm_bytes_sent(c) - sent0 - wire[0];
    if ((rc = adopt_region(R, total))) return rc;
    R.s_adopt = R.clock.lap();
    const OverlapBooks &tb = R.tuple_books, &rb = R.region_books;
    if (R.clock.on)
        std::fprintf(stderr,
                     "[shard timing] rank %d/%d tuples in %d chunks: extraction + owner partition %.4f s, exchange %.4f s of which %.4f s beside the next chunk's "
                     "extraction (loop %.4f s, %llu B out), owner layout %.4f s, K2-K4 %.4f s; regions %s: selections for %d ranks %.4f s, exchange %.4f s of which "
                     "%.4f s beside the next selection (loop %.4f s, %llu B out), owner order %.4f s, import+region+release %.4f s\n",
                     R.me, R.W, R.C, tb.step, tb.xfer, tb.hidden, tb.loop, (unsigned long long)wire[0], R.s_layout, R.s_build, pipeline ? "pipelined" : "whole", R.W,
                     rb.step, rb.xfer, rb.hidden, rb.loop, (unsigned long long)wire[1], R.s_owner_order, R.s_adopt);
    return PAG_OK;
}
}  // namespace

extern "C" int pag_shard_run(pag_graph *g, pag_comm *c, const pag_build_input *in, const pag_region *regions, pag_build_stats *total) {
    if (!g || !c || !in || !regions) return PAG_EINVAL;
    const int rc = shard_run(g, c, in, regions, total);
    if (rc != PAG_OK) pag_comm_abort(c, pag_last_error());  // the peers learn why instead of waiting for this rank
    return rc;
}

