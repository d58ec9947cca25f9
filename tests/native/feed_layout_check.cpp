// feed_layout_check -- the arenas and pinned blocks of mcevidence_amd/csrc/feed_layout.hpp on the CPU (tests/test_feed_layout_shared.py).
//   feed_layout_check all
// Grid: every field of FeedArena / FeedPinned / PrefixArena / PrefixPinned starts on a multiple of its alignment, the fields follow one
// another in the declared order without overlap, each holds its documented content (written to, under AddressSanitizer, wherever the
// arena is small enough to allocate), the sizing pass and the placing pass agree, and lam | status lie side by side.
// Pins: at six named tuples per arena, dev_bytes, host_bytes and every offset are those of the library at f000f58, the last commit
// whose feed_plan / prefix_plan counted the offsets by hand (the numbers were printed by a copy of those lines; -1: the field is absent).
// Prints "ok feed=<count> prefix=<count> pins=<count>" last; the first failed check prints its line and ends the run with status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "feed_layout.hpp"

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fprintf(stderr, "%s:%d: check failed: %s  [%s, field %s]\n", __FILE__, __LINE__, #cond, g_where, g_field); \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

using namespace mce_feed;
static char g_where[256] = "";
static const char* g_field = "-";

struct Field {
    const char* name;
    const void* p;
    size_t bytes, align;      // the documented content; the alignment its start must have
};

// fields in the declared order; null pointers are absent fields
static void check_fields(const std::vector<Field>& f, char* base, size_t total, bool touch)
{
    size_t end = 0;
    for (size_t i = 0; i < f.size(); ++i) {
        if (!f[i].p) continue;
        const size_t off = (size_t)(static_cast<const char*>(f[i].p) - base);
        g_field = f[i].name;
        CHECK(off % f[i].align == 0);
        CHECK(off >= end);                    // behind everything before it: order and no overlap
        CHECK(off + f[i].bytes <= total);
        end = off + f[i].bytes;
        if (touch && f[i].bytes) memset(base + off, 0x5a, f[i].bytes);
    }
    g_field = "-";
}

static void check_back(const EigBack& b, int d, int nsys, int stat_ints)
{
    CHECK(reinterpret_cast<const char*>(b.status) == reinterpret_cast<const char*>(b.lam) + (size_t)nsys * d * sizeof(double));
    CHECK(b.bytes == (size_t)nsys * (d * sizeof(double) + stat_ints * sizeof(int32_t)));
    CHECK(b.lam_at(nsys - 1) == b.lam + (size_t)(nsys - 1) * d && b.status_at(nsys - 1) == b.status + (size_t)(nsys - 1) * stat_ints);
}

static std::vector<Field> feed_dev_fields(const FeedArena& a, const FeedSizes& z)
{
    const size_t D = sizeof(double), dd = (size_t)z.d * z.d, ns = (size_t)z.nsys;
    std::vector<Field> f = {{"S1", a.S1, (size_t)z.n1 * z.d * D, 256}, {"S2", a.S2, (size_t)(z.ntot - z.n1) * z.d * D, 8},
                            {"W", a.W, (size_t)z.n1 * D, 256}, {"F", a.F, (size_t)z.n1 * D, 256}, {"O", a.O, (size_t)z.kmax * D, 256},
                            {"mean3", a.mean3, kMean3 * D, 256}, {"cov", a.cov, dd * D, 8}, {"evec", a.evec, dd * D, 8}, {"scale", a.scale, z.d * D, 8},
                            {"sum", a.sum, 8, 8}, {"part", a.part, z.part_doubles * D, 256}, {"ws", a.ws, z.search_ws_bytes, 256},
                            {"vdist", a.vdist, (size_t)z.n1 * z.K * D, 256}, {"vws", a.vws, z.verify_ws_bytes, 256}, {"vres", a.vres, 2 * sizeof(int32_t), 256},
                            {"e_cov", a.eig.cov, ns * dd * D, 256}, {"e_evec", a.eig.evec, ns * dd * D, 8}, {"e_scale", a.eig.scale, ns * z.d * D, 8},
                            {"e_lam", a.eig.back.lam, ns * z.d * D, 8}, {"e_status", a.eig.back.status, ns * z.stat_ints * sizeof(int32_t), 8}};
    return f;
}

static std::vector<Field> feed_host_fields(const FeedPinned& h, const FeedSizes& z)
{
    const size_t D = sizeof(double), dd = (size_t)z.d * z.d, ns = (size_t)z.nsys;
    return {{"cov", h.cov, 2 * dd * D, 8}, {"evec", h.evec, 2 * dd * D, 8}, {"scale", h.scale, 2 * z.d * D, 8}, {"dotp", h.dotp, z.kmax * D, 8},
            {"sum", h.sum, 8, 8}, {"verify", h.verify, 2 * sizeof(int), 4}, {"lam", h.eig.lam, ns * z.d * D, 8},
            {"status", h.eig.status, ns * z.stat_ints * sizeof(int32_t), 4}};
}

static std::vector<Field> prefix_dev_fields(const PrefixArena& a, const PrefixSizes& z)
{
    const size_t D = sizeof(double), dd = (size_t)z.d * z.d, ns = (size_t)z.nsys;
    return {{"S1", a.S1, (size_t)z.n1 * z.d * D, 256}, {"S2", a.S2, (size_t)(z.ntot - z.n1) * z.d * D, 8},
            {"X", a.X, z.own_systems ? (size_t)z.pmax * z.d * D : 0, 256}, {"W", a.W, (size_t)z.n1 * D, 256}, {"L", a.L, (size_t)z.n1 * D, 256},
            {"F", a.F, (size_t)z.pmax * D, 256}, {"P", a.P, z.B * sizeof(int64_t), 256}, {"lmax", a.lmax, z.B * D, 256},
            {"blk", a.blk, (size_t)z.B * z.nblk_max * D, 256}, {"O", a.O, (size_t)z.B * z.kmax * D, 256}, {"mean3", a.mean3, kMean3 * D, 256},
            {"evec", a.evec, dd * D, 8}, {"scale", a.scale, z.d * D, 8}, {"cov", a.cov, ns * dd * D, 8}, {"part", a.part, z.part_doubles * D, 256},
            {"ws", a.ws, z.search_ws_bytes, 256}, {"vdist", a.vdist, (size_t)z.vrows * z.K * D, 256}, {"vws", a.vws, z.verify_ws_bytes, 256},
            {"vres", a.vres, (size_t)z.nsearch * 2 * sizeof(int32_t), 256}, {"dpart", a.dpart, z.cross ? (size_t)z.B * z.nblk_dotp * z.kmax * D : 0, 256},
            {"e_evec", a.eig.evec, ns * dd * D, 256}, {"e_scale", a.eig.scale, ns * z.d * D, 8}, {"e_lam", a.eig.back.lam, ns * z.d * D, 8},
            {"e_status", a.eig.back.status, ns * z.stat_ints * sizeof(int32_t), 8}};
}

static std::vector<Field> prefix_host_fields(const PrefixPinned& h, const PrefixSizes& z)
{
    const size_t D = sizeof(double), dd = (size_t)z.d * z.d, ns = (size_t)z.nsys;
    return {{"sys", h.sys, ns * dd * D, 8}, {"scale", h.scale, ns * z.d * D, 8}, {"dotp", h.dotp, (size_t)z.B * z.kmax * D, 8}, {"lmax", h.lmax, z.B * D, 8},
            {"verify", h.verify, (size_t)z.nsearch * 2 * sizeof(int), 4}, {"lam", h.eig.lam, ns * z.d * D, 8},
            {"status", h.eig.status, ns * z.stat_ints * sizeof(int32_t), 4}};
}

// arenas up to this size are allocated and every field written to; larger ones are checked by their offsets from a base that is never read
constexpr size_t kTouchMax = (size_t)4 << 20;
static char* const kFakeBase = reinterpret_cast<char*>((size_t)1 << 32);

template <class Arena, class Sizes, class Fields> static Arena place(const Sizes& z, size_t align, Fields fields)
{
    const size_t total = Arena(z).total;          // the sizing pass
    CHECK(total % (align == 256 ? 256 : 64) == 0);
    const bool touch = total <= kTouchMax;
    char* base = touch ? static_cast<char*>(aligned_alloc(align == 256 ? 256 : 64, total)) : kFakeBase;
    CHECK(base != nullptr);
    const Arena a(z, base);
    CHECK(a.total == total);
    check_fields(fields(a, z), base, total, touch);
    if (touch) free(base);
    return Arena(z, kFakeBase);
}

static long long g_feed = 0, g_prefix = 0;

static void check_feed(const FeedSizes& z)
{
    snprintf(g_where, sizeof(g_where), "feed n1=%lld ntot=%lld d=%d kmax=%d K=%d nsys=%d nverify=%d dev_eig=%d", (long long)z.n1, (long long)z.ntot, z.d, z.kmax,
             z.K, z.nsys, z.nverify, (int)z.dev_eig);
    const FeedArena a = place<FeedArena>(z, 256, feed_dev_fields);
    const FeedPinned h = place<FeedPinned>(z, 8, feed_host_fields);
    CHECK((a.vdist != nullptr) == (z.nverify > 0) && (a.eig.evec != nullptr) == z.dev_eig && (h.eig.lam != nullptr) == z.dev_eig);
    CHECK(a.S2 == a.S1 + (size_t)z.n1 * z.d);
    if (z.dev_eig) {
        check_back(a.eig.back, z.d, z.nsys, z.stat_ints);
        check_back(h.eig, z.d, z.nsys, z.stat_ints);
        CHECK(a.eig.back.bytes == h.eig.bytes);
        CHECK(a.eig.cov_at(z.nsys - 1) + (size_t)z.d * z.d == a.eig.evec && a.eig.evec_at(z.nsys - 1) + (size_t)z.d * z.d == a.eig.scale &&
              a.eig.scale_at(z.nsys - 1) + z.d == a.eig.back.lam);
    }
    CHECK(h.cov_at(1) + (size_t)z.d * z.d == h.evec && h.evec_at(1) + (size_t)z.d * z.d == h.scale && h.scale_at(1) + z.d == h.dotp);
    ++g_feed;
}

static void check_prefix(const PrefixSizes& z)
{
    snprintf(g_where, sizeof(g_where), "prefix n1=%lld ntot=%lld pmax=%lld d=%d kmax=%d B=%d nsearch=%d nsys=%d own=%d cross=%d dev_eig=%d", (long long)z.n1,
             (long long)z.ntot, (long long)z.pmax, z.d, z.kmax, z.B, z.nsearch, z.nsys, (int)z.own_systems, (int)z.cross, (int)z.dev_eig);
    const PrefixArena a = place<PrefixArena>(z, 256, prefix_dev_fields);
    const PrefixPinned h = place<PrefixPinned>(z, 8, prefix_host_fields);
    CHECK((a.eig.evec != nullptr) == z.dev_eig && (h.eig.lam != nullptr) == z.dev_eig);
    CHECK(a.S2 == a.S1 + (size_t)z.n1 * z.d && a.cov_at(1) == a.cov + (size_t)z.d * z.d);
    if (z.dev_eig) {
        check_back(a.eig.back, z.d, z.nsys, z.stat_ints);
        check_back(h.eig, z.d, z.nsys, z.stat_ints);
        CHECK(a.eig.back.bytes == h.eig.bytes && a.eig.cov == a.cov);          // the solver reads the slots the covariance kernels filled
    }
    CHECK(h.sys_at(z.nsys) == h.scale && h.scale_at(z.nsys) == h.dotp);
    ++g_prefix;
}

struct FeedPin {
    const char* name;
    FeedSizes z;
    size_t dev_bytes, host_bytes;
    long long dev[20], host[8];
};
struct PrefixPin {
    const char* name;
    PrefixSizes z;
    size_t dev_bytes, host_bytes;
    long long dev[24], host[7];
};

// n1, ntot, d, kmax, K, nsys, nverify, stat_ints, dev_eig, part_doubles, search_ws_bytes, verify_ws_bytes
static const FeedPin kFeedPins[6] = {
    {"auto_small", {40, 40, 3, 3, 2, 1, 0, 4, false, 49152, 12345, 0}, 409856, 384,
     {0, 960, 1024, 1536, 2048, 2304, 3840, 3912, 3984, 4008, 4096, 397312, -1, -1, -1, -1, -1, -1, -1, -1},
     {0, 144, 288, 336, 360, 368, -1, -1}},
    {"auto_verify", {513, 513, 27, 10, 9, 1, 256, 4, false, 96768, 1000001, 18432}, 1963520, 23872,
     {0, 110808, 110848, 115200, 119552, 119808, 121344, 127176, 133008, 133224, 133376, 907520, 1907712, 1944832, 1963264, -1, -1, -1, -1, -1},
     {0, 11664, 23328, 23760, 23840, 23848, -1, -1}},
    {"cross_all_dev", {513, 543, 63, 3, 3, 1, 1, 4, true, 516096, 777, 256}, 4556288, 128576,
     {0, 258552, 273920, 278272, 282624, 282880, 284416, 316168, 347920, 348424, 348672, 4477440, 4478464, 4491008, 4491264, 4491520, 4523272, 4555024, 4555528, 4556032},
     {0, 63504, 127008, 128016, 128040, 128048, 128056, 128560}},
    {"cross_single_d127_dev", {40, 70, 127, 33, 33, 2, 0, 4, true, 2080768, 65536, 0}, 17565696, 520512,
     {0, 40640, 71168, 71680, 72192, 72704, 74240, 203272, 332304, 333320, 333568, 16979712, -1, -1, -1, 17045248, 17303312, 17561376, 17563408, 17565440},
     {0, 258064, 516128, 518160, 518424, 518432, 518440, 520472}},
    {"cross_single_host_whiten", {2, 3, 64, 2, 2, 2, 1, 4, false, 532480, 0, 256}, 4330752, 132160,
     {0, 1024, 1536, 1792, 2048, 2304, 3840, 36608, 69376, 69888, 70144, 4329984, 4329984, 4330240, 4330496, -1, -1, -1, -1, -1},
     {0, 65536, 131072, 132096, 132112, 132120, -1, -1}},
    {"auto_d1_dev_verify", {5000, 5000, 1, 2, 1, 1, 256, 4, true, 49152, 769, 2048}, 559616, 128,
     {0, 40000, 40192, 80384, 120576, 120832, 122368, 122376, 122384, 122392, 122624, 515840, 516864, 557056, 559104, 559360, 559368, 559376, 559384, 559392},
     {0, 16, 32, 48, 64, 72, 80, 88}},
};

// n1, ntot, pmax, vrows, d, kmax, K, B, nsearch, nsys, nblk_max, nblk_dotp, stat_ints, own_systems, cross, dev_eig, part_doubles, search_ws_bytes, verify_ws_bytes
static const PrefixPin kPrefixPins[6] = {
    {"auto_all_b1", {40, 40, 40, 0, 3, 3, 2, 1, 1, 1, 1, 1, 4, false, false, false, 49152, 12345, 0}, 411392, 192,
     {0, 960, 1024, 1024, 1536, 2048, 2560, 2816, 3072, 3328, 3584, 5120, 5192, 5216, 5376, 398592, 411136, 411136, 411136, 411392, -1, -1, -1, -1},
     {0, 72, 96, 120, 128, -1, -1}},
    {"auto_all_b3_verify", {513, 513, 513, 513, 27, 10, 9, 3, 2, 1, 1, 3, 4, false, false, false, 96768, 1000001, 18432}, 1968640, 6336,
     {0, 110808, 110848, 110848, 115200, 119552, 123904, 124160, 124416, 124672, 124928, 126464, 132296, 132512, 138496, 912640, 1912832, 1949952, 1968384, 1968640, -1, -1, -1, -1},
     {0, 5832, 6048, 6288, 6312, -1, -1}},
    {"auto_single_b3_dev", {513, 513, 500, 500, 63, 3, 2, 3, 3, 3, 1, 2, 4, true, false, true, 516096, 777, 256}, 4890880, 98496,
     {0, 258552, 258560, 510720, 515072, 519424, 523520, 523776, 524032, 524288, 524544, 526080, 557832, 558336, 653824, 4782592, 4783616, 4791808, 4792064, 4792320, 4792320, 4887576, 4889088, 4890600},
     {0, 95256, 96768, 96840, 96864, 96896, 98408}},
    {"auto_single_d127_dev", {5000, 5000, 5000, 5000, 127, 33, 32, 2, 2, 2, 5, 20, 4, true, false, true, 2080768, 65536, 65536}, 28992000, 262784,
     {0, 5080000, 5080064, 10160128, 10200320, 10240512, 10280704, 10280960, 10281216, 10281472, 10282240, 10283776, 10412808, 10413824, 10672128, 27318272, 27383808, 28663808, 28729344, 28729600, 28729600, 28987664, 28989696, 28991728},
     {0, 258064, 260096, 260624, 260640, 260664, 262696}},
    {"cross_b256", {513, 543, 513, 513, 64, 2, 2, 256, 1, 1, 1, 3, 4, false, true, false, 532480, 4097, 0}, 4654080, 39488,
     {0, 262656, 278016, 278016, 282368, 286720, 291072, 293120, 295168, 297216, 301312, 302848, 335616, 336128, 368896, 4628736, 4633088, 4641536, 4641536, 4641792, -1, -1, -1, -1},
     {0, 32768, 33280, 37376, 39424, -1, -1}},
    {"cross_b256_dev_d1", {5000, 5001, 4999, 4999, 1, 10, 10, 256, 1, 1, 5, 20, 4, false, true, true, 49152, 1, 20480}, 1421568, 22592,
     {0, 40000, 40192, 40192, 80384, 120576, 160768, 162816, 164864, 175104, 195584, 197120, 197128, 197136, 197376, 590592, 590848, 990976, 1011456, 1011712, 1421312, 1421320, 1421328, 1421336},
     {0, 8, 16, 20496, 22544, 22560, 22568}},
};

static void check_pin(const std::vector<Field>& f, const long long* want, size_t nwant)
{
    CHECK(f.size() == nwant);
    for (size_t i = 0; i < nwant; ++i) {
        g_field = f[i].name;
        const long long got = f[i].p ? (long long)(static_cast<const char*>(f[i].p) - kFakeBase) : -1;
        CHECK(got == want[i]);
    }
    g_field = "-";
}

int main(int argc, char**)
{
    if (argc < 2) {
        fprintf(stderr, "usage: feed_layout_check all\n");
        return 1;
    }
    const int D[5] = {1, 2, 63, 64, 127}, N1[3] = {2, 40, 513}, N2[3] = {0, 1, 30}, KM[3] = {2, 3, 33}, BS[3] = {1, 3, 256};
    const int kStat = 4;
    for (int d : D)
        for (int n1 : N1)
            for (int n2 : N2)
                for (int kmax : KM)
                    for (int nverify = 0; nverify <= 1; ++nverify)
                        for (int dev = 0; dev <= 1; ++dev) {
                            const int K = kmax - (n2 ? 0 : 1);
                            // sizes that are no multiple of anything, so that every take has to round
                            const size_t part = (size_t)3 * d + 7, wsb = (size_t)1000 * kmax + n1 + 1, vws = nverify ? (size_t)2 * K * 4 * nverify : 0;
                            for (int nsys = 1; nsys <= (n2 ? 2 : 1); ++nsys) {
                                FeedSizes z;
                                z.n1 = n1; z.ntot = n1 + n2; z.d = d; z.kmax = kmax; z.K = K; z.nsys = nsys; z.nverify = nverify; z.stat_ints = kStat;
                                z.dev_eig = dev != 0; z.part_doubles = part; z.search_ws_bytes = wsb; z.verify_ws_bytes = vws;
                                check_feed(z);
                            }
                            for (int B : BS) {
                                // equal neighbouring sizes: {p}, {p, p, n1}, pairs of equal sizes
                                const int nd = B == 1 ? 1 : B == 3 ? 2 : B / 2;
                                for (int own = 0; own <= (n2 ? 0 : 1); ++own) {
                                    PrefixSizes z;
                                    z.n1 = n1; z.ntot = n1 + n2; z.pmax = n1 > 2 ? n1 - 1 : n1; z.d = d; z.kmax = kmax; z.K = K; z.B = B;
                                    z.cross = n2 != 0; z.own_systems = own != 0;
                                    z.nsearch = z.cross ? 1 : nd; z.nsys = own ? nd : 1;
                                    z.vrows = (z.cross || nverify) ? z.pmax : 0;
                                    z.nblk_max = (int)((z.pmax + 1023) / 1024); z.nblk_dotp = (int)((z.pmax + 255) / 256);
                                    z.stat_ints = kStat; z.dev_eig = dev != 0; z.part_doubles = part; z.search_ws_bytes = wsb; z.verify_ws_bytes = vws;
                                    check_prefix(z);
                                }
                            }
                        }
    long long pins = 0;
    for (const FeedPin& p : kFeedPins) {
        snprintf(g_where, sizeof(g_where), "pin %s", p.name);
        const FeedArena a(p.z, kFakeBase);
        const FeedPinned h(p.z, kFakeBase);
        CHECK(a.total == p.dev_bytes && FeedArena(p.z).total == p.dev_bytes);
        CHECK(h.total == p.host_bytes && FeedPinned(p.z).total == p.host_bytes);
        check_pin(feed_dev_fields(a, p.z), p.dev, 20);
        check_pin(feed_host_fields(h, p.z), p.host, 8);
        check_feed(p.z);
        ++pins;
    }
    for (const PrefixPin& p : kPrefixPins) {
        snprintf(g_where, sizeof(g_where), "pin %s", p.name);
        const PrefixArena a(p.z, kFakeBase);
        const PrefixPinned h(p.z, kFakeBase);
        CHECK(a.total == p.dev_bytes && PrefixArena(p.z).total == p.dev_bytes);
        CHECK(h.total == p.host_bytes && PrefixPinned(p.z).total == p.host_bytes);
        check_pin(prefix_dev_fields(a, p.z), p.dev, 24);
        check_pin(prefix_host_fields(h, p.z), p.host, 7);
        check_prefix(p.z);
        ++pins;
    }
    printf("ok feed=%lld prefix=%lld pins=%lld\n", g_feed, g_prefix, pins);
    return 0;
}
