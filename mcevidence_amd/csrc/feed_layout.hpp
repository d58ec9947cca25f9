// feed_layout.hpp -- where everything of one evidence-feed job lies: the device arenas and the pinned host blocks of the feed
// (capi_feed.hpp) and of its convergence batches (capi_prefix.hpp).  Each is declared ONCE, as a row of WsPlan takes like SumWs /
// MarWs, and here the row IS the member list: a field's line declares it, places it and says what it holds, in the order of the
// memory.  The sizes come in as plain numbers (what the search, the re-check and the covariance kernels need: as bytes and doubles);
// without a base a constructor only sizes (`total`), with one it also leaves the typed pointers.  Host only, plain C++17, no device
// header: tests/native/feed_layout_check.cpp compiles it on the CPU and pins it to the offsets the library had when they were counted
// by hand.  Every device array starts on a multiple of 256 bytes (the kernels' vector loads rely on it); a block whose parts are read
// together is ONE such array, its parts 8 bytes aligned inside it.  The pinned blocks are 8 bytes aligned inside, a multiple of 64 long.
#pragma once
#include <cstddef>
#include <cstdint>

#include "ws_plan.hpp"

namespace mce_feed {

constexpr size_t kSub = 8;
constexpr int kMean3 = 3 * 64;        // doubles of the covariance kernels' mean / min / max block

// what the device eigen-solver hands back for nsys systems, in ONE copy of `bytes`: lam [nsys][d] | status [nsys][stat_ints]
struct EigBack {
    int d = 0, stat_ints = 0;
    double* lam = nullptr;
    int32_t* status = nullptr;
    size_t bytes = 0;
    EigBack() = default;
    EigBack(WsPlan& P, int d_, int nsys, int stat_ints_) : d(d_), stat_ints(stat_ints_), bytes(P.total)
    {
        lam = P.take<double>((size_t)nsys * d);
        status = P.take<int32_t>((size_t)nsys * stat_ints);
        bytes = P.total - bytes;
    }
    double* lam_at(int i) const { return lam + (size_t)i * d; }
    int32_t* status_at(int i) const { return status + (size_t)i * stat_ints; }
};

// the device eigen-solver's slots, one block, nsys of each: [cov |] evec | scale | lam | status.  The feed keeps the covariances in
// the block (own_cov); the convergence batches have theirs elsewhere and set `cov` themselves.
struct EigSlots {
    int d = 0;
    double *cov = nullptr, *evec = nullptr, *scale = nullptr;
    EigBack back;
    EigSlots() = default;
    EigSlots(WsPlan& P, int d_, int nsys, int stat_ints, bool own_cov) : d(d_)
    {
        WsPlan Q(P.here(), kSub);
        if (own_cov) cov = Q.take<double>((size_t)nsys * d * d);
        evec = Q.take<double>((size_t)nsys * d * d);
        scale = Q.take<double>((size_t)nsys * d);
        back = EigBack(Q, d, nsys, stat_ints);
        P.take_bytes<char>(Q.total);
    }
    double* cov_at(int i) const { return cov + (size_t)i * d * d; }
    double* evec_at(int i) const { return evec + (size_t)i * d * d; }
    double* scale_at(int i) const { return scale + (size_t)i * d; }
};

// ---- the feed: one problem of mce_evidence_feed_batch_f64 ----
struct FeedSizes {
    int64_t n1 = 0, ntot = 0;           // rows of s1; of s1 U s2
    int d = 0, kmax = 0, K = 0;
    int nsys = 1;                       // eigen-systems: 2 for a 'single' cross evidence
    int nverify = 0;                    // rows the certificate re-checks (0: none, and none of its three arrays)
    int stat_ints = 0;                  // mce_eig::kStatInts
    bool dev_eig = false;               // the device eigen-solver: its slots behind everything else
    size_t part_doubles = 0, search_ws_bytes = 0, verify_ws_bytes = 0;
};

struct FeedArena {
    FeedSizes z;
    WsPlan P;
    double* S1 = P.take<double>((size_t)z.ntot * z.d);                  // the rows [ntot][d], whitened in place ...
    double* S2 = S1 ? S1 + (size_t)z.n1 * z.d : nullptr;                // ... s2 behind s1
    double* W = P.take<double>((size_t)z.n1);                           // weights
    double* F = P.take<double>((size_t)z.n1);                           // likelihood terms
    double* O = P.take<double>((size_t)z.kmax);                         // the sums
    WsPlan Q{P.here(), kSub};                                           // one block: mean3 | cov | evec | scale | checksum
    double* mean3 = Q.take<double>(kMean3);
    double* cov = Q.take<double>((size_t)z.d * z.d);
    double* evec = Q.take<double>((size_t)z.d * z.d);
    double* scale = Q.take<double>((size_t)z.d);
    unsigned long long* sum = Q.take<unsigned long long>(1);
    char* block = P.take_bytes<char>(Q.total);
    double* part = P.take<double>(z.part_doubles);                      // the covariance / mean kernels' partials
    char* ws = P.take_bytes<char>(z.search_ws_bytes);                   // the search's workspace
    double* vdist = z.nverify > 0 ? P.take<double>((size_t)z.n1 * z.K) : nullptr;           // the certificate: distances [n1][K],
    char* vws = z.nverify > 0 ? P.take_bytes<char>(z.verify_ws_bytes) : nullptr;            // its workspace,
    int32_t* vres = z.nverify > 0 ? P.take<int32_t>(2) : nullptr;                           // {rows checked, rows failed}
    EigSlots eig = z.dev_eig ? EigSlots(P, z.d, z.nsys, z.stat_ints, true) : EigSlots();
    size_t total = P.total;
    explicit FeedArena(const FeedSizes& sizes = FeedSizes(), void* base = nullptr) : z(sizes), P(base) {}
};

// a job's slice of the pinned arena: what comes back from the device, and the host's eigen-systems on their way up
struct FeedPinned {
    FeedSizes z;
    WsPlan P;
    double* cov = P.take<double>((size_t)2 * z.d * z.d);                // two systems' worth, whatever nsys is
    double* evec = P.take<double>((size_t)2 * z.d * z.d);
    double* scale = P.take<double>((size_t)2 * z.d);
    double* dotp = P.take<double>((size_t)z.kmax);
    unsigned long long* sum = P.take<unsigned long long>(1);
    int* verify = P.take<int>(2);                                       // {rows checked, rows failed}
    EigBack eig = z.dev_eig ? EigBack(P, z.d, z.nsys, z.stat_ints) : EigBack();
    size_t total = (P.total + 63) & ~(size_t)63;
    explicit FeedPinned(const FeedSizes& sizes = FeedSizes(), void* base = nullptr) : z(sizes), P(base, kSub) {}
    double* cov_at(int i) const { return cov + (size_t)i * z.d * z.d; }
    double* evec_at(int i) const { return evec + (size_t)i * z.d * z.d; }
    double* scale_at(int i) const { return scale + (size_t)i * z.d; }
};

// ---- the convergence batches: one call of mce_evidence_feed_prefix_f64 ----
struct PrefixSizes {
    int64_t n1 = 0, ntot = 0, pmax = 0; // rows of s1; of s1 U s2; of the longest prefix
    int64_t vrows = 0;                  // rows whose distances are kept (the certificate; cross: the reductions read them)
    int d = 0, kmax = 0, K = 0, B = 0;
    int nsearch = 0, nsys = 0;          // searches; eigen-systems (cov_mode 1: one per distinct prefix)
    int nblk_max = 0, nblk_dotp = 0;    // workgroups of prefix_max_kernel / prefix_dotp_kernel
    int stat_ints = 0;
    bool own_systems = false;           // cov_mode 1: every prefix whitened out of place by its own system
    bool cross = false, dev_eig = false;
    size_t part_doubles = 0, search_ws_bytes = 0, verify_ws_bytes = 0;
};

struct PrefixArena {
    PrefixSizes z;
    WsPlan Pl;
    double* S1 = Pl.take<double>((size_t)z.ntot * z.d);                 // as the feed's
    double* S2 = S1 ? S1 + (size_t)z.n1 * z.d : nullptr;
    double* X = Pl.take<double>(z.own_systems ? (size_t)z.pmax * z.d : 0);          // own_systems: the whitened prefix [pmax][d]
    double* W = Pl.take<double>((size_t)z.n1);                          // weights
    double* L = Pl.take<double>((size_t)z.n1);                          // log-likelihoods
    double* F = Pl.take<double>((size_t)z.pmax);                        // likelihood terms of the prefix being searched
    int64_t* P = Pl.take<int64_t>((size_t)z.B);                         // the prefix sizes
    double* lmax = Pl.take<double>((size_t)z.B);                        // the shifts
    double* blk = Pl.take<double>((size_t)z.B * z.nblk_max);            // their partials
    double* O = Pl.take<double>((size_t)z.B * z.kmax);                  // the sums
    WsPlan Q{Pl.here(), kSub};                                          // one block: mean3 | evec | scale | cov [nsys]
    double* mean3 = Q.take<double>(kMean3);
    double* evec = Q.take<double>((size_t)z.d * z.d);
    double* scale = Q.take<double>((size_t)z.d);
    double* cov = Q.take<double>((size_t)z.nsys * z.d * z.d);
    char* block = Pl.take_bytes<char>(Q.total);
    double* part = Pl.take<double>(z.part_doubles);
    char* ws = Pl.take_bytes<char>(z.search_ws_bytes);
    double* vdist = Pl.take<double>((size_t)z.vrows * z.K);
    char* vws = Pl.take_bytes<char>(z.verify_ws_bytes);
    int32_t* vres = Pl.take<int32_t>((size_t)z.nsearch * 2);            // [nsearch][2]
    double* dpart = Pl.take<double>(z.cross ? (size_t)z.B * z.nblk_dotp * z.kmax : 0);      // cross: [B][nblk_dotp][kmax]
    EigSlots eig = z.dev_eig ? EigSlots(Pl, z.d, z.nsys, z.stat_ints, false) : EigSlots();  // the device solver's output; it solves `cov`
    size_t total = Pl.total;
    explicit PrefixArena(const PrefixSizes& sizes = PrefixSizes(), void* base = nullptr) : z(sizes), Pl(base) { eig.cov = cov; }
    double* cov_at(int i) const { return cov + (size_t)i * z.d * z.d; }
};

struct PrefixPinned {
    PrefixSizes z;
    WsPlan P;
    double* sys = P.take<double>((size_t)z.nsys * z.d * z.d);           // the covariances; the host's eigenvectors replace them in place
    double* scale = P.take<double>((size_t)z.nsys * z.d);
    double* dotp = P.take<double>((size_t)z.B * z.kmax);
    double* lmax = P.take<double>((size_t)z.B);
    int* verify = P.take<int>((size_t)z.nsearch * 2);                   // [nsearch][2]
    double* spare = P.take<double>(1);                                  // (one double the block has always had: host_bytes stays what it was)
    EigBack eig = z.dev_eig ? EigBack(P, z.d, z.nsys, z.stat_ints) : EigBack();
    size_t total = (P.total + 63) & ~(size_t)63;
    explicit PrefixPinned(const PrefixSizes& sizes = PrefixSizes(), void* base = nullptr) : z(sizes), P(base, kSub) {}
    double* sys_at(int i) const { return sys + (size_t)i * z.d * z.d; }
    double* scale_at(int i) const { return scale + (size_t)i * z.d; }
};

}  // namespace mce_feed
