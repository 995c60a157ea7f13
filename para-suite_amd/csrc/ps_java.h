// ps_java.h -- the rules of the Java toolkit (and of htsjdk under it) that more than one mode restates: how a double or a
// float prints, Integer.parseInt, String.split, and the reference bases a CIGAR covers.  Host only, no HIP include; what a
// kernel calls too is __host__ __device__ when the HIP compiler reads this.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#ifdef __HIPCC__
#define PS_JAVA_HD __host__ __device__ inline
#else
#define PS_JAVA_HD inline
#endif

namespace ps {

// java.lang.Double.toString / Float.toString: the shortest decimal that reads back as the same value (the JDK 19+
// definition; older JDKs print a longer digit string for a few values), plain notation with at least one fraction digit for
// 1e-3 <= |v| < 1e7, otherwise d.dddE<exp>
template <class T> std::string java_fp_to_string(T v)
{
    constexpr bool wide = std::is_same<T, double>::value;
    static_assert(wide || std::is_same<T, float>::value, "double or float");
    if (v != v) return "NaN";
    if (std::isinf(v)) return v > 0 ? "Infinity" : "-Infinity";
    if (v == 0) return std::signbit(v) ? "-0.0" : "0.0";
    char buf[64];
    for (int prec = 1; prec <= (wide ? 17 : 9); ++prec) {
        std::snprintf(buf, sizeof buf, "%.*e", prec - 1, (double)v);
        if ((wide ? (T)std::strtod(buf, nullptr) : (T)std::strtof(buf, nullptr)) == v) break;
    }
    std::string m(buf); const size_t ep = m.find('e');
    const int e10 = std::atoi(m.c_str() + ep + 1);
    std::string digits; bool neg = false;
    for (size_t i = 0; i < ep; ++i) { if (m[i] == '-') neg = true; else if (m[i] >= '0' && m[i] <= '9') digits.push_back(m[i]); }
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    std::string o = neg ? "-" : "";
    const T av = std::fabs(v);
    if (av >= (T)1e-3 && av < (T)1e7) {
        if (e10 >= 0) {
            std::string ip = digits.substr(0, std::min(digits.size(), (size_t)e10 + 1));
            while ((int)ip.size() < e10 + 1) ip.push_back('0');
            o += ip + "." + (digits.size() > (size_t)e10 + 1 ? digits.substr((size_t)e10 + 1) : "0");
        } else o += "0." + std::string((size_t)(-e10 - 1), '0') + digits;
    } else o += digits.substr(0, 1) + "." + (digits.size() > 1 ? digits.substr(1) : "0") + "E" + std::to_string(e10);
    return o;
}
inline std::string java_double_to_string(double v) { return java_fp_to_string(v); }
inline std::string java_float_to_string(float v) { return java_fp_to_string(v); }

// Integer.parseInt on ASCII: one optional sign, at least one digit, the value in int32 range
PS_JAVA_HD bool java_parse_int(const uint8_t *s, uint32_t n, int32_t &v)
{
    uint32_t i = 0; bool neg = false;
    if (n && (s[0] == '-' || s[0] == '+')) { neg = s[0] == '-'; i = 1; }
    if (i >= n) return false;
    unsigned long long x = 0;
    for (; i < n; ++i) {
        if (s[i] < '0' || s[i] > '9') return false;
        x = x * 10 + (unsigned long long)(s[i] - '0');
        if (x > 2147483648ull) return false;                              // leading zeros are fine, so the length says nothing
    }
    if (!neg && x > 2147483647ull) return false;
    v = (int32_t)(neg ? 0u - (uint32_t)x : (uint32_t)x);
    return true;
}

inline bool java_parse_int(const std::string &s, int32_t &v) { return java_parse_int((const uint8_t *)s.data(), (uint32_t)s.size(), v); }

// Boolean.parseBoolean: "true" in any letter case; everything else, the empty string included, is false
inline bool java_parse_boolean(const std::string &s)
{
    static const char t[] = "true";
    if (s.size() != 4) return false;
    for (int i = 0; i < 4; ++i) if ((s[i] | 0x20) != t[i]) return false;
    return true;
}

// Double.parseDouble on its decimal forms: white space at either end trimmed (String.trim: everything up to ' '), one optional sign,
// "NaN", "Infinity", or digits with an optional point and exponent, one optional suffix d D f F.  Hexadecimal floating-point
// literals, which the Java also reads, are refused
inline bool java_parse_double(const std::string &text, double &v)
{
    size_t a = 0, b = text.size();
    while (a < b && (unsigned char)text[a] <= ' ') ++a;
    while (b > a && (unsigned char)text[b - 1] <= ' ') --b;
    std::string s = text.substr(a, b - a);
    if (s.empty()) return false;
    size_t i = s[0] == '-' || s[0] == '+' ? 1 : 0;
    const bool neg = s[0] == '-';
    const std::string body = s.substr(i);
    if (body == "NaN") { v = std::nan(""); return true; }
    if (body == "Infinity") { v = neg ? -INFINITY : INFINITY; return true; }
    if (body.size() > 1 && (body.back() == 'd' || body.back() == 'D' || body.back() == 'f' || body.back() == 'F')) s.pop_back();
    bool digit = false;
    for (size_t k = i; k < s.size(); ++k) {
        const char c = s[k];
        if (c >= '0' && c <= '9') digit = true;
        else if (c != '.' && c != 'e' && c != 'E' && c != '+' && c != '-') return false;
    }
    if (!digit) return false;
    char *end = nullptr;
    const double x = std::strtod(s.c_str(), &end);
    if (end != s.c_str() + s.size()) return false;
    v = x;
    return true;
}

// String.split(sep): trailing empty strings are dropped, an empty input is one empty string
inline std::vector<std::string> java_split(const std::string &s, char sep)
{
    std::vector<std::string> out; size_t p = 0;
    for (;;) { const size_t q = s.find(sep, p); if (q == std::string::npos) { out.push_back(s.substr(p)); break; } out.push_back(s.substr(p, q - p)); p = q + 1; }
    if (s.empty()) return out;
    while (!out.empty() && out.back().empty()) out.pop_back();
    return out;
}

// the reference bases a CIGAR covers (htsjdk getAlignmentEnd - getAlignmentStart + 1): M, D, N, = and X of MIDNSHP=X
PS_JAVA_HD bool cigar_on_ref(int op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
PS_JAVA_HD int64_t cigar_ref_span(const uint32_t *words, uint32_t n)
{
    int64_t span = 0;
    for (uint32_t k = 0; k < n; ++k) if (cigar_on_ref((int)(words[k] & 15u))) span += words[k] >> 4;
    return span;
}

}  // namespace ps
