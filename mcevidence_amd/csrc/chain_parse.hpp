// chain_parse.hpp -- one numeric token of a chain text file -> the correctly rounded fp64 value, shared by the host reader
// (chain_reader.cpp, plain C++17 under g++) and the device reader (chain_kernels.hpp, __host__ __device__ under hipcc).
//
// Two layers:
//   * host and device: scan_decimal (sign, digits, point, exponent -> a 64-bit decimal mantissa and a power of ten), clinger_exact
//     (Clinger's fast path: mantissa <= 2^53 and |e10| <= 22, or 22 < e10 <= 37 while the mantissa absorbs the excess -- ONE
//     correctly rounded IEEE multiply or divide) and eisel_lemire (up to 19 significant digits, any exponent: the 64-bit mantissa
//     times a 128-bit truncated power of five, high words only).  Each returns the correctly rounded double or says that it
//     cannot decide; none of them ever returns a wrong value.
//   * host only: parse_slow (strtod_l in the C locale: inf, nan, near-halfway products, long tails, subnormals, overflow, junk) and
//     parse_token, exactly what the host reader has always called: the fast path, then strtod.
// The HOST reader calls clinger_exact and strtod only; the DEVICE reader adds eisel_lemire and leaves the undecided tokens to the
// host's strtod -- so the two readers stay independent witnesses of each other in the tests.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MCE_HD __host__ __device__
#else
#define MCE_HD
#endif

#include <locale.h>

#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace mce_parse {

MCE_HD inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\v' || c == '\f'; }
MCE_HD inline bool is_digit(char c) { return c >= '0' && c <= '9'; }

// what a conversion step says about a token
enum : int {
    kRejected = -1,   // not a number in any spelling strtod accepts as a whole token
    kUndecided = 0,   // this step cannot tell: the next one (in the end the host's strtod) must
    kConverted = 1    // *out holds the correctly rounded value
};

// sign * mant * 10^e10; inexact: digits beyond the 64-bit mantissa were dropped and at least one of them is not zero
struct Decimal {
    uint64_t mant = 0;
    int e10 = 0;
    bool neg = false, inexact = false;
};

// [p, e) -> Decimal.  kUndecided: no digits at all (inf / nan / junk: strtod's business).  kRejected: an exponent without digits or
// bytes after the number.  The token must be shorter than 2^30 bytes (the readers cap it at 4096).
MCE_HD inline int scan_decimal(const char* p, const char* e, Decimal& v)
{
    if (p < e && (*p == '+' || *p == '-')) {
        v.neg = (*p == '-');
        ++p;
    }
    uint64_t mant = 0;
    int shift = 0;           // decimal exponent adjustment from the digits themselves
    bool any = false, inexact = false;
    constexpr uint64_t kMantMax = (UINT64_MAX - 9) / 10;
    while (p < e && is_digit(*p)) {
        any = true;
        if (mant <= kMantMax) mant = mant * 10 + (uint64_t)(*p - '0');
        else { ++shift; inexact |= (*p != '0'); }
        ++p;
    }
    if (p < e && *p == '.') {
        ++p;
        while (p < e && is_digit(*p)) {
            any = true;
            if (mant <= kMantMax) { mant = mant * 10 + (uint64_t)(*p - '0'); --shift; }
            else inexact |= (*p != '0');
            ++p;
        }
    }
    if (!any) return kUndecided;
    int e10 = 0;
    if (p < e && (*p == 'e' || *p == 'E')) {
        ++p;
        bool eneg = false;
        if (p < e && (*p == '+' || *p == '-')) { eneg = (*p == '-'); ++p; }
        if (p == e || !is_digit(*p)) return kRejected;
        while (p < e && is_digit(*p)) {
            if (e10 < 100000) e10 = e10 * 10 + (*p - '0');
            ++p;
        }
        if (eneg) e10 = -e10;
    }
    if (p != e) return kRejected;
    v.mant = mant;
    v.e10 = e10 + shift;
    v.inexact = inexact;
    return kConverted;
}

MCE_HD inline double pow10_exact(int i)          // 10^i, 0 <= i <= 22: exactly representable
{
    switch (i) {
    case 0: return 1e0;   case 1: return 1e1;   case 2: return 1e2;   case 3: return 1e3;   case 4: return 1e4;   case 5: return 1e5;
    case 6: return 1e6;   case 7: return 1e7;   case 8: return 1e8;   case 9: return 1e9;   case 10: return 1e10; case 11: return 1e11;
    case 12: return 1e12; case 13: return 1e13; case 14: return 1e14; case 15: return 1e15; case 16: return 1e16; case 17: return 1e17;
    case 18: return 1e18; case 19: return 1e19; case 20: return 1e20; case 21: return 1e21; default: return 1e22;
    }
}

// Clinger's exact fast path
MCE_HD inline int clinger_exact(const Decimal& v, double* out)
{
    if (v.inexact || v.mant > ((uint64_t)1 << 53)) return kUndecided;
    if (v.mant == 0) { *out = v.neg ? -0.0 : 0.0; return kConverted; }
    double d = (double)v.mant;
    const int e10 = v.e10;
    if (e10 >= -22 && e10 <= 22) {
        d = e10 < 0 ? d / pow10_exact(-e10) : d * pow10_exact(e10);
        *out = v.neg ? -d : d;
        return kConverted;
    }
    if (e10 > 22 && e10 <= 22 + 15) {               // mant * 10^(e10-22) still exact below 2^53
        d *= pow10_exact(e10 - 22);
        if (d <= 9007199254740992.0) {
            d *= pow10_exact(22);
            *out = v.neg ? -d : d;
            return kConverted;
        }
    }
    return kUndecided;
}

// ---- Eisel-Lemire ---------------------------------------------------------------------------------------------------------
// (D. Lemire, "Number parsing at a gigabyte per second", 2021; the table and the rounding rules are those of the public
// fast_float / Go strconv implementations.)  pow5[2 (q - kPow5Min)], [.. + 1]: high and low word of the 128 most significant
// bits of 5^q -- truncated for q >= 0, of the reciprocal rounded up for q < 0.  make_pow5_table() below fills it.
constexpr int kPow5Min = -342, kPow5Max = 308;
constexpr int kPow5Words = 2 * (kPow5Max - kPow5Min + 1);

MCE_HD inline uint64_t mul64(uint64_t a, uint64_t b, uint64_t* hi)
{
#if defined(__HIP_DEVICE_COMPILE__)
    *hi = __umul64hi(a, b);
    return a * b;
#else
    const unsigned __int128 r = (unsigned __int128)a * b;
    *hi = (uint64_t)(r >> 64);
    return (uint64_t)r;
#endif
}

// w * 10^q for 0 < w < 2^64 exactly known: the correctly rounded NORMAL double (sign not applied), or kUndecided (results that are
// zero, subnormal or infinite, and the rare products the 128-bit table cannot settle)
MCE_HD inline int eisel_lemire_u64(uint64_t w, int q, const uint64_t* pow5, double* out)
{
    if (w == 0 || q < kPow5Min || q > kPow5Max) return kUndecided;
    const int lz = __builtin_clzll(w);
    w <<= lz;
    const uint64_t* t = pow5 + 2 * (q - kPow5Min);
    uint64_t hi, lo = mul64(w, t[0], &hi);
    constexpr uint64_t kPrecisionMask = UINT64_MAX >> 55;          // 52 explicit mantissa bits + 3
    if ((hi & kPrecisionMask) == kPrecisionMask) {                 // the low word of the table could carry into the bits that matter
        uint64_t hi2;
        (void)mul64(w, t[1], &hi2);
        lo += hi2;
        if (hi2 > lo) ++hi;
    }
    // the truncated table leaves the last bit of a product that ends in all ones open outside the range where 5^|q| (or its
    // reciprocal) is exact in 128 bits
    if (lo == UINT64_MAX && !(q >= -27 && q <= 55)) return kUndecided;
    const int upperbit = (int)(hi >> 63);
    const int shift = upperbit + 64 - 52 - 3;
    uint64_t mant = hi >> shift;
    // floor(log2(10^q)) + 63 = ((152170 + 65536) q >> 16) + 63 for |q| <= 342
    int power2 = (int)(((int64_t)(152170 + 65536) * q) >> 16) + 63 + upperbit - lz + 1023;
    if (power2 <= 0) return kUndecided;                            // subnormal or zero
    // exactly halfway between two doubles (possible only for 5^q < 2^64 dividing the mantissa): round to even
    if (lo <= 1 && q >= -4 && q <= 23 && (mant & 3) == 1 && (mant << shift) == hi) mant &= ~(uint64_t)1;
    mant += (mant & 1);
    mant >>= 1;
    if (mant >= ((uint64_t)2 << 52)) {
        mant = (uint64_t)1 << 52;
        ++power2;
    }
    mant &= ~((uint64_t)1 << 52);
    if (power2 >= 0x7FF) return kUndecided;                        // infinity
    const uint64_t bits = mant | ((uint64_t)power2 << 52);
    double d;
    __builtin_memcpy(&d, &bits, sizeof(d));
    *out = d;
    return kConverted;
}

// a scanned decimal: exact mantissas directly; a mantissa with dropped digits lies in (mant, mant + 1) x 10^e10, so where both
// ends round to the same double that double is the answer
MCE_HD inline int eisel_lemire(const Decimal& v, const uint64_t* pow5, double* out)
{
    double d;
    if (eisel_lemire_u64(v.mant, v.e10, pow5, &d) != kConverted) return kUndecided;
    if (v.inexact) {
        double d1;
        if (v.mant == UINT64_MAX || eisel_lemire_u64(v.mant + 1, v.e10, pow5, &d1) != kConverted || d1 != d) return kUndecided;
    }
    *out = v.neg ? -d : d;
    return kConverted;
}

// the host reader's conversion without strtod: Clinger's fast path only
MCE_HD inline int parse_token_fast(const char* p, const char* e, double* out)
{
    Decimal v;
    const int rc = scan_decimal(p, e, v);
    return rc == kConverted ? clinger_exact(v, out) : rc;
}

// the device reader's conversion: the fast path, then Eisel-Lemire
MCE_HD inline int parse_token_exact(const char* p, const char* e, const uint64_t* pow5, double* out)
{
    Decimal v;
    const int rc = scan_decimal(p, e, v);
    if (rc != kConverted) return rc;
    if (clinger_exact(v, out) == kConverted) return kConverted;
    return eisel_lemire(v, pow5, out);
}

// ---- host only ------------------------------------------------------------------------------------------------------------
constexpr size_t kMaxTokenBytes = 4096;

inline locale_t c_locale()
{
    static locale_t loc = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    return loc;
}

// strtod on a copy of the token; accepts what Python's float() accepts for decimal text
inline bool parse_slow(const char* p, const char* e, double* out)
{
    const size_t n = (size_t)(e - p);
    if (n == 0 || n > kMaxTokenBytes) return false;
    for (const char* q = p; q < e; ++q) {
        const char c = *q;
        const bool ok = is_digit(c) || c == '+' || c == '-' || c == '.' || c == 'e' || c == 'E' ||
                        ((c | 0x20) >= 'a' && (c | 0x20) <= 'z' && (c | 0x20) != 'x' && (c | 0x20) != 'p');
        if (!ok) return false;
    }
    char buf[kMaxTokenBytes + 4];
    std::memcpy(buf, p, n);
    buf[n] = '\0';
    char* endp = nullptr;
    errno = 0;
    const double v = strtod_l(buf, &endp, c_locale());
    if (endp != buf + n) return false;
    *out = v;
    return true;
}

// one numeric token [p, e) -> correctly rounded double
inline bool parse_token(const char* p, const char* e, double* out)
{
    const int rc = parse_token_fast(p, e, out);
    if (rc != kUndecided) return rc == kConverted;
    return parse_slow(p, e, out);
}

// The table of eisel_lemire_u64, made with schoolbook arithmetic on 32-bit limbs (little endian):
//   q >= 0: 5^q shifted left until bit 127 is set, or right (truncating) until it fits 128 bits;
//   q <  0: floor(2^b / 5^-q) + 1 with b = z + 127 (q >= -27) or 2 z + 128 (below), z = bits of 5^-q rounded up to the next power of
//           two's exponent, then truncated to 128 bits.
namespace detail {
using Big = std::vector<uint32_t>;
inline void trim(Big& a) { while (!a.empty() && a.back() == 0) a.pop_back(); }
inline void mul_small(Big& a, uint32_t m)
{
    uint64_t c = 0;
    for (auto& x : a) { c += (uint64_t)x * m; x = (uint32_t)c; c >>= 32; }
    if (c) a.push_back((uint32_t)c);
}
inline int bit_length(const Big& a) { return a.empty() ? 0 : (int)(32 * (a.size() - 1)) + 32 - __builtin_clz(a.back()); }
inline bool bit(const Big& a, int i) { return (size_t)(i >> 5) < a.size() && ((a[(size_t)(i >> 5)] >> (i & 31)) & 1u); }
inline int cmp(const Big& a, const Big& b)
{
    if (a.size() != b.size()) return a.size() < b.size() ? -1 : 1;
    for (size_t i = a.size(); i-- > 0;)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return 0;
}
inline void sub(Big& a, const Big& b)          // a -= b, a >= b
{
    int64_t c = 0;
    for (size_t i = 0; i < a.size(); ++i) {
        c += (int64_t)a[i] - (i < b.size() ? (int64_t)b[i] : 0);
        a[i] = (uint32_t)c;
        c >>= 32;
    }
    trim(a);
}
inline void shl1_or(Big& a, bool low)          // a = 2 a + low
{
    uint32_t c = low ? 1u : 0u;
    for (auto& x : a) { const uint32_t n = x >> 31; x = (x << 1) | c; c = n; }
    if (c) a.push_back(c);
}
// bits [lo, lo + 128) of a -> hi, lo words
inline void take128(const Big& a, int lo, uint64_t* out)
{
    uint64_t w[2] = {0, 0};
    for (int i = 0; i < 128; ++i)
        if (lo + i >= 0 && bit(a, lo + i)) w[i >> 6] |= (uint64_t)1 << (i & 63);
    out[0] = w[1];
    out[1] = w[0];
}
inline void add_one(Big& a)
{
    for (auto& x : a)
        if (++x != 0) return;
    a.push_back(1);
}
}  // namespace detail

inline void make_pow5_table(uint64_t* table /* [kPow5Words] */)
{
    using namespace detail;
    Big p{1};
    for (int q = 0; q <= kPow5Max; ++q) {           // 5^q, its 128 leading bits
        const int n = bit_length(p);
        if (n >= 128) take128(p, n - 128, table + 2 * (q - kPow5Min));
        else {
            Big s(p);
            for (int i = n; i < 128; ++i) shl1_or(s, false);
            take128(s, 0, table + 2 * (q - kPow5Min));
        }
        mul_small(p, 5);
    }
    p = Big{1};
    for (int q = -1; q >= kPow5Min; --q) {
        mul_small(p, 5);                            // 5^-q
        int z = bit_length(p);                      // smallest z with 2^z >= 5^-q (5^k is never a power of two for k > 0)
        const int b = q >= -27 ? z + 127 : 2 * z + 128;
        Big quo, rem;                               // 2^b / p by shift and subtract
        quo.assign((size_t)(b / 32 + 1), 0);
        for (int i = b; i >= 0; --i) {
            shl1_or(rem, i == b);
            if (cmp(rem, p) >= 0) {
                sub(rem, p);
                quo[(size_t)(i >> 5)] |= 1u << (i & 31);
            }
        }
        trim(quo);
        add_one(quo);
        const int n = bit_length(quo);
        take128(quo, n - 128, table + 2 * (q - kPow5Min));
    }
}

inline const uint64_t* pow5_table()
{
    static const std::vector<uint64_t> t = [] {
        std::vector<uint64_t> v((size_t)kPow5Words);
        make_pow5_table(v.data());
        return v;
    }();
    return t.data();
}

}  // namespace mce_parse
