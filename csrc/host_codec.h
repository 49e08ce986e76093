// Host side of the /score request path, free of torch, pybind and HIP so that
// it also compiles into a stand-alone program (tests/host/codec_harness.cpp,
// run under AddressSanitizer and UBSan): the JSON request parser, the
// response writer and the drift p-value epilogue. creditcore_kernels.hip
// includes this header and keeps the Python-facing wrappers.
#pragma once

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

// ---------------------------------------------------------------------------
// encode_json — parse a /score request body (JSON bytes, the wire format:
// [{"sex": "male", ..., "credit_limit": 18000.0, ...}, ...]) straight into
// (codes, nums) with no intermediate Python objects. This is the serving
// fast path; any deviation from the expected shape throws and the caller
// falls back to the pydantic path for a proper 422.
// ---------------------------------------------------------------------------

// Off the accepted path: kept out of line so that the per-field loop stays small.
#define HOST_CODEC_COLD __attribute__((noinline, cold))

namespace jsonenc {

struct Error {
  std::string msg;
};

struct Parser {
  const char* p;
  const char* end;

  [[noreturn]] HOST_CODEC_COLD void fail(const char* what) {
    throw Error{std::string(what) + " at offset " + std::to_string((size_t)(p - begin_))};
  }
  const char* begin_;

  void ws() {
    while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) ++p;
  }
  bool eat(char c) {
    ws();
    if (p < end && *p == c) { ++p; return true; }
    return false;
  }
  void expect(char c, const char* what) {
    if (!eat(c)) fail(what);
  }

  // Parse a JSON string starting at the opening quote; returns the raw
  // span between quotes and whether it contains escapes. Fast path: one
  // SIMD memchr to the closing quote + one over the span for backslashes
  // (escapes are rare in this schema's values).
  void raw_string(const char*& s, size_t& len, bool& escaped) {
    expect('"', "expected string");
    s = p;
    const char* q = (const char*)std::memchr(p, '"', (size_t)(end - p));
    if (q == nullptr) { p = end; fail("unterminated string"); }
    if (std::memchr(p, '\\', (size_t)(q - p)) == nullptr) {
      escaped = false;
      len = (size_t)(q - s);
      p = q + 1;
      return;
    }
    escaped = true;
    while (p < end) {
      const char c = *p;
      if (c == '"') { len = (size_t)(p - s); ++p; return; }
      if (c == '\\') {
        ++p;
        if (p >= end) break;
      }
      ++p;
    }
    fail("unterminated string");
  }

  // What JSON allows between the quotes, escapes aside: no control byte and
  // well-formed UTF-8 (no overlong form, no surrogate, nothing past
  // U+10FFFF). A string that matched a schema key or a vocabulary word byte
  // for byte needs no such check; every other string gets it, so that a body
  // the pydantic path answers with 422 is not answered with 200 here.
  static bool valid_text(const char* s, size_t len) {
    const unsigned char* u = (const unsigned char*)s;
    size_t i = 0;
    while (i < len) {
      const unsigned c = u[i];
      if (c < 0x80) {
        if (c < 0x20) return false;
        ++i;
        continue;
      }
      size_t n;  // continuation bytes
      unsigned lo = 0x80, hi = 0xBF;  // range of the first of them
      if (c >= 0xC2 && c <= 0xDF) n = 1;
      else if (c == 0xE0) { n = 2; lo = 0xA0; }
      else if (c == 0xED) { n = 2; hi = 0x9F; }
      else if (c >= 0xE1 && c <= 0xEF) n = 2;
      else if (c == 0xF0) { n = 3; lo = 0x90; }
      else if (c == 0xF4) { n = 3; hi = 0x8F; }
      else if (c >= 0xF1 && c <= 0xF3) n = 3;
      else return false;
      if (len - i <= n) return false;
      if (u[i + 1] < lo || u[i + 1] > hi) return false;
      for (size_t k = 2; k <= n; ++k)
        if ((u[i + k] & 0xC0) != 0x80) return false;
      i += n + 1;
    }
    return true;
  }

  // Unescape the span between the quotes. Returns SIZE_MAX for an escape
  // that JSON does not have (an unknown letter, \u without four hex digits,
  // a surrogate without its partner); otherwise the unescaped length, of
  // which the first min(length, cap) bytes are in buf. A result longer than
  // cap is valid but equals no key or vocabulary word.
  static size_t unescape(const char* s, size_t len, char* buf, size_t cap) {
    size_t o = 0;
    auto put = [&](unsigned ch) {
      if (o < cap) buf[o] = (char)ch;
      ++o;
    };
    auto hex4 = [&](size_t at, unsigned& cp) {  // s[at .. at + 3]
      if (at > len || len - at < 4) return false;
      cp = 0;
      for (size_t k = at; k < at + 4; ++k) {
        const char h = s[k];
        cp <<= 4;
        if (h >= '0' && h <= '9') cp |= (unsigned)(h - '0');
        else if (h >= 'a' && h <= 'f') cp |= (unsigned)(h - 'a' + 10);
        else if (h >= 'A' && h <= 'F') cp |= (unsigned)(h - 'A' + 10);
        else return false;
      }
      return true;
    };
    for (size_t i = 0; i < len; ++i) {
      if (s[i] != '\\') { put((unsigned char)s[i]); continue; }
      if (++i >= len) return SIZE_MAX;
      switch (s[i]) {
        case '"': put('"'); break;
        case '\\': put('\\'); break;
        case '/': put('/'); break;
        case 'b': put('\b'); break;
        case 'f': put('\f'); break;
        case 'n': put('\n'); break;
        case 'r': put('\r'); break;
        case 't': put('\t'); break;
        case 'u': {
          unsigned cp;
          if (!hex4(i + 1, cp)) return SIZE_MAX;
          i += 4;  // now at the last hex digit
          if (cp >= 0xDC00 && cp <= 0xDFFF) return SIZE_MAX;  // low half first
          if (cp >= 0xD800 && cp <= 0xDBFF) {
            unsigned low;
            if (len - i < 7 || s[i + 1] != '\\' || s[i + 2] != 'u' || !hex4(i + 3, low) ||
                low < 0xDC00 || low > 0xDFFF)
              return SIZE_MAX;
            i += 6;
            cp = 0x10000 + ((cp - 0xD800) << 10) + (low - 0xDC00);
          }
          if (cp < 0x80) {
            put(cp);
          } else if (cp < 0x800) {
            put(0xC0 | (cp >> 6));
            put(0x80 | (cp & 0x3F));
          } else if (cp < 0x10000) {
            put(0xE0 | (cp >> 12));
            put(0x80 | ((cp >> 6) & 0x3F));
            put(0x80 | (cp & 0x3F));
          } else {
            put(0xF0 | (cp >> 18));
            put(0x80 | ((cp >> 12) & 0x3F));
            put(0x80 | ((cp >> 6) & 0x3F));
            put(0x80 | (cp & 0x3F));
          }
          break;
        }
        default: return SIZE_MAX;
      }
    }
    return o;
  }

  // A string off the fast lane (escaped, or equal to no key or word): fail
  // unless it is valid JSON text. Returns the unescaped length (see above).
  HOST_CODEC_COLD size_t checked(const char* s, size_t len, bool escaped, char* buf, size_t cap) {
    if (!valid_text(s, len)) fail("control byte or malformed UTF-8 in string");
    if (!escaped) return len;
    const size_t n = unescape(s, len, buf, cap);
    if (n == SIZE_MAX) fail("bad escape in string");
    return n;
  }

  // JSON's number grammar, -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?,
  // is narrower than what std::from_chars takes: that also reads nan, inf,
  // nan(...), 01, 1. and .5. So the span it consumed is checked: it starts
  // with a digit after the optional sign (no nan, inf or .5), a leading 0
  // stands alone (no 01), and a '.' has a digit behind it (no 1. or 1.e5).
  // from_chars stops before an exponent without digits, which then fails as
  // trailing bytes. A value outside the double range is left to the fallback.
  double number() {
    ws();
    double v;
    auto [q, ec] = std::from_chars(p, end, v);
    if (ec != std::errc()) fail("expected number");
    auto digit = [](char c) { return c >= '0' && c <= '9'; };
    const char* s = p + (*p == '-');
    if (s >= q || !digit(*s)) fail("expected number");
    if (*s == '0' && s + 1 < q && digit(s[1])) fail("leading zero in number");
    const char* dot = (const char*)std::memchr(s, '.', (size_t)(q - s));
    if (dot != nullptr && (dot + 1 >= q || !digit(dot[1]))) fail("digit expected after '.'");
    p = q;
    return v;
  }

  bool literal(const char* lit) {
    const size_t n = std::strlen(lit);
    if ((size_t)(end - p) >= n && std::memcmp(p, lit, n) == 0) { p += n; return true; }
    return false;
  }

  // Deepest nesting taken inside an ignored value; the pydantic path gives
  // up at a depth of its own, above this one plus the two levels around it.
  static constexpr int kMaxSkipDepth = 64;

  void skip_string() {
    const char* s; size_t l; bool e;
    raw_string(s, l, e);
    char none[1];
    checked(s, l, e, none, 0);
  }

  // Step over the value of an ignored field. It is still validated in full
  // (brackets matched by kind, commas and colons in place, strings, numbers
  // and literals well-formed): the pydantic path rejects the whole body for
  // an error inside a field it would otherwise ignore.
  HOST_CODEC_COLD void skip_value() {
    char kind[kMaxSkipDepth];
    int depth = 0;
    for (;;) {
      ws();
      if (p >= end) fail("truncated value");
      const char c = *p;
      bool opened = false;
      if (c == '{' || c == '[') {
        if (depth == kMaxSkipDepth) fail("ignored value nested too deep");
        kind[depth++] = c;
        ++p;
        if (c == '{') {
          if (eat('}')) {
            --depth;
          } else {
            skip_string();
            expect(':', "expected ':'");
            opened = true;
          }
        } else if (eat(']')) {
          --depth;
        } else {
          opened = true;
        }
      } else if (c == '"') {
        skip_string();
      } else if (literal("null") || literal("true") || literal("false")) {
      } else {
        number();
      }
      if (opened) continue;  // the container's first value comes next
      // a value has ended: close containers until one goes on
      for (;;) {
        if (depth == 0) return;
        if (kind[depth - 1] == '[') {
          if (eat(',')) break;
          expect(']', "expected ',' or ']'");
        } else {
          if (eat(',')) {
            skip_string();
            expect(':', "expected ':'");
            break;
          }
          expect('}', "expected ',' or '}'");
        }
        --depth;
      }
    }
  }
};

}  // namespace jsonenc

#undef HOST_CODEC_COLD

// Persistent encoder state: column dispatch table keyed by
// (key_len << 8) | last_char — one int hash + at most a couple of memcmp
// per field instead of hashing 15-18-char strings 23k times per request.
struct JsonEncoderState {
  std::vector<std::string> key_store;
  std::unordered_map<uint32_t, std::vector<std::pair<int, int>>> dispatch;
  // dispatch value: (key_store index, column id)
  std::vector<std::vector<std::string>> vocab;
  std::vector<int16_t> missing_code;
  std::vector<int16_t> def_codes;
  std::vector<float> def_nums;
  int ncat{}, nnum{};

  JsonEncoderState(std::vector<std::vector<std::string>> vocabs,
                   const std::vector<std::string>& cat_names,
                   const std::vector<std::string>& num_names,
                   const std::string& missing_cat,
                   std::vector<int16_t> default_codes,
                   std::vector<float> default_nums)
      : vocab(std::move(vocabs)),
        def_codes(std::move(default_codes)),
        def_nums(std::move(default_nums)) {
    ncat = (int)cat_names.size();
    nnum = (int)num_names.size();
    if ((int)vocab.size() != ncat)
      throw std::invalid_argument("one vocabulary per categorical column");
    if ((int)def_codes.size() != ncat || (int)def_nums.size() != nnum)
      throw std::invalid_argument("default row size mismatch");
    missing_code.assign(ncat, -1);
    for (int j = 0; j < ncat; ++j) {
      key_store.push_back(cat_names[j]);
      for (size_t k = 0; k < vocab[j].size(); ++k)
        if (vocab[j][k] == missing_cat) missing_code[j] = (int16_t)k;
    }
    for (int j = 0; j < nnum; ++j) key_store.push_back(num_names[j]);
    for (int j = 0; j < ncat + nnum; ++j) {
      const std::string& k = key_store[j];
      if (k.empty()) throw std::invalid_argument("empty column name");
      const uint32_t h = ((uint32_t)k.size() << 8) | (uint8_t)k.back();
      dispatch[h].emplace_back(j, j);
    }
  }

  inline int lookup(const char* ks, size_t kl) const {
    if (kl == 0) return -1;
    const uint32_t h = ((uint32_t)kl << 8) | (uint8_t)ks[kl - 1];
    auto it = dispatch.find(h);
    if (it == dispatch.end()) return -1;
    for (const auto& cand : it->second) {
      const std::string& name = key_store[cand.first];
      if (name.size() == kl && std::memcmp(name.data(), ks, kl) == 0)
        return cand.second;
    }
    return -1;
  }
};

// Parse the full body into flat row-major code/num vectors. Takes no Python
// object, so callers release the GIL around it. Throws jsonenc::Error on
// malformed input.
inline size_t parse_records_nogil(const JsonEncoderState& st, const char* data,
                                  ptrdiff_t blen, std::vector<int16_t>& codes,
                                  std::vector<float>& nums) {
  const int ncat = st.ncat;
  const int nnum = st.nnum;
  const auto& vocab = st.vocab;
  const int16_t* def_codes = st.def_codes.data();
  const float* def_nums = st.def_nums.data();
  size_t b = 0;
  {
    jsonenc::Parser P{data, data + blen};
    P.begin_ = data;
    codes.reserve((size_t)blen / 70 * ncat + ncat);
    nums.reserve((size_t)blen / 70 * nnum + nnum);
    {
      P.expect('[', "body must be a JSON array");
      if (!P.eat(']')) {
        do {
          P.expect('{', "record must be an object");
          codes.resize(codes.size() + ncat);
          nums.resize(nums.size() + nnum);
          int16_t* crow = codes.data() + b * ncat;
          float* nrow = nums.data() + b * nnum;
          // absent fields take the schema defaults (pydantic semantics,
          // reference app/model.py:8-34)
          std::memcpy(crow, def_codes, ncat * sizeof(int16_t));
          std::memcpy(nrow, def_nums, nnum * sizeof(float));
          // clients overwhelmingly emit fields in schema order (pydantic
          // model dumps, the sample request, pandas records): try the
          // expected next column with one memcmp before the hash lookup
          int expect_col = 0;
          if (!P.eat('}')) {
            do {
              const char* ks; size_t kl; bool kesc;
              P.raw_string(ks, kl, kesc);
              char kbuf[64];
              if (kesc) {
                // a key longer than the buffer is no schema key: kl = 0
                const size_t n = P.checked(ks, kl, true, kbuf, sizeof(kbuf));
                ks = kbuf; kl = (n <= sizeof(kbuf)) ? n : 0;
              }
              P.expect(':', "expected ':'");
              int col = -1;
              if (expect_col < ncat + nnum) {
                const std::string& exp = st.key_store[expect_col];
                if (exp.size() == kl && std::memcmp(exp.data(), ks, kl) == 0)
                  col = expect_col;
              }
              if (col < 0) col = st.lookup(ks, kl);
              expect_col = (col >= 0) ? col + 1 : expect_col;
              if (col < 0) {
                if (!kesc) P.checked(ks, kl, false, nullptr, 0);
                P.skip_value();  // extra fields ignored (schema extra="ignore")
              } else if (col < ncat) {
                const int j = col;
                P.ws();
                if (P.p < P.end && *P.p == 'n') {
                  P.fail("null not accepted for a string field");
                } else {
                  const char* vs; size_t vl; bool vesc;
                  P.raw_string(vs, vl, vesc);
                  char vbuf[64];
                  if (vesc) {
                    vl = P.checked(vs, vl, true, vbuf, sizeof(vbuf));
                    vs = vbuf;
                  }
                  int16_t code = -1;  // unknown category -> all-zero one-hot
                  if (vl <= sizeof(vbuf) || !vesc) {
                    for (size_t k = 0; k < vocab[j].size(); ++k) {
                      const std::string& cand = vocab[j][k];
                      if (cand.size() == vl && std::memcmp(cand.data(), vs, vl) == 0) {
                        code = (int16_t)k;
                        break;
                      }
                    }
                  }
                  if (code < 0 && !vesc) P.checked(vs, vl, false, nullptr, 0);
                  crow[j] = code;
                }
              } else {
                const int j = col - ncat;
                P.ws();
                if (P.p < P.end && *P.p == 'n') {
                  P.fail("null not accepted for a numeric field");
                } else {
                  nrow[j] = (float)P.number();
                }
              }
            } while (P.eat(','));
            P.expect('}', "expected '}'");
          }
          ++b;
        } while (P.eat(','));
        P.expect(']', "expected ']'");
      }
      P.ws();
      if (P.p != P.end) P.fail("trailing data");
    }
  }
  return b;
}

// ---------------------------------------------------------------------------
// Drift p-value epilogue on host, in C: chi-square survival via the exact
// closed forms for integer dof (even: Poisson tail sum; odd: erfc +
// half-integer-gamma series, both from the Q(k+2) = Q(k) + term recurrence)
// and the Pelz-Good series for the two-sample K-S p-value (mirrors
// creditcore.models.drift._pelz_good_sf; validated against scipy in
// tests/test_drift_pvals_host.py).
// Replaces ~0.4 ms of numpy/scipy per request with ~5 µs on the Pelz-Good
// path (en >= 300, the serving batch sizes). Small batches cost more: the
// exact matrix (en <= 140, and tiny D below en = 500) and the Smirnov sum
// (140 < en < 300, up to en terms per drifted column) are not timed here.
// ---------------------------------------------------------------------------

inline double chi2_sf_int_dof(double x, int dof) {
  if (dof <= 0) return 1.0;
  if (x <= 0.0) return 1.0;
  // Q(1) = erfc(sqrt(x/2)); Q(2) = exp(-x/2);
  // Q(k+2) = Q(k) + (x/2)^(k/2) e^(-x/2) / Gamma(k/2 + 1)
  const double h = 0.5 * x;
  double q, term;
  int k;
  if (dof % 2 == 1) {
    q = std::erfc(std::sqrt(h));
    term = std::sqrt(h / M_PI) * std::exp(-h) * 2.0;  // k=1 increment
    k = 1;
  } else {
    q = std::exp(-h);
    term = h * std::exp(-h);  // k=2 increment
    k = 2;
  }
  while (k + 2 <= dof) {
    q += term;
    k += 2;
    term *= h / (0.5 * k);
  }
  return std::min(1.0, std::max(0.0, q));
}

// Exact P(D_n > d) for small n via the Marsaglia-Tsang-Wang (2003) matrix
// method (Durbin's matrix, one of the exact algorithms scipy's kstwo picks
// from). k-d band is small in practice (k ~ ceil(n d) ~ sqrt(n) near the
// null); the sf underflows to 0 for n d^2 > 18 long before m gets large.
inline double mtw_sf(int n, double d) {
  if (d <= 0.0) return 1.0;
  if (d >= 1.0) return 0.0;
  if (n * d * d > 18.0) return 0.0;  // sf < ~2e-16
  const int k = (int)std::ceil(n * d);
  const double h = k - n * d;
  const int m = 2 * k - 1;
  std::vector<double> H((size_t)m * m, 0.0), Q((size_t)m * m, 0.0), tmp((size_t)m * m);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j)
      if (i - j + 1 >= 0) H[(size_t)i * m + j] = 1.0;
  for (int i = 0; i < m; ++i) {
    H[(size_t)i * m] -= std::pow(h, i + 1);
    H[(size_t)(m - 1) * m + i] -= std::pow(h, m - i);
  }
  H[(size_t)(m - 1) * m] += (2 * h - 1 > 0 ? std::pow(2 * h - 1, m) : 0.0);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j)
      if (i - j + 1 > 0)
        for (int g = 1; g <= i - j + 1; ++g) H[(size_t)i * m + j] /= g;
  // Q = H^n with power-of-two scaling to avoid under/overflow
  int eH = 0, eQ = 0;
  auto matmul = [&](const std::vector<double>& a, const std::vector<double>& b,
                    std::vector<double>& c) {
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) {
        double s = 0.0;
        for (int g = 0; g < m; ++g) s += a[(size_t)i * m + g] * b[(size_t)g * m + j];
        c[(size_t)i * m + j] = s;
      }
  };
  auto rescale = [&](std::vector<double>& a, int& e) {
    if (a[(size_t)(k - 1) * m + (k - 1)] > 1e140) {
      for (auto& v : a) v *= 1e-140;
      e += 140;
    }
  };
  // initialize Q = I
  for (int i = 0; i < m; ++i) Q[(size_t)i * m + i] = 1.0;
  int nn = n;
  while (nn > 0) {
    if (nn & 1) {
      matmul(Q, H, tmp);
      Q.swap(tmp);
      eQ += eH;
      rescale(Q, eQ);
    }
    matmul(H, H, tmp);
    H.swap(tmp);
    eH *= 2;
    rescale(H, eH);
    nn >>= 1;
  }
  double s = Q[(size_t)(k - 1) * m + (k - 1)];
  // multiply by n! / n^n with the same scaling discipline
  for (int i = 1; i <= n; ++i) {
    s *= (double)i / n;
    if (s < 1e-140) {
      s *= 1e140;
      eQ -= 140;
    }
  }
  const double cdf = s * std::pow(10.0, eQ);
  return std::min(1.0, std::max(0.0, 1.0 - cdf));
}

inline double pelz_good_sf(double x, double n) {
  if (x <= 0.0) return 1.0;
  if (x >= 1.0) return 0.0;
  const double z = std::sqrt(n) * x;
  const double z2 = z * z, z3 = z2 * z, z4 = z2 * z2, z6 = z4 * z2;
  const double z7 = z6 * z, z8 = z4 * z4, z10 = z8 * z2;
  const double PI2 = M_PI * M_PI, PI4 = PI2 * PI2, PI6 = PI4 * PI2;
  const double SQRT2PI = std::sqrt(2.0 * M_PI);

  const double qlog = -PI2 / 8.0 / z2;
  if (qlog < -690.0) return 1.0;  // cdf ~ 0
  const double q = std::exp(qlog);

  const double k1a = -z2, k1b = PI2 / 4.0;
  const double k2a = 6 * z6 + 2 * z4;
  const double k2b = (2 * z4 - 5 * z2) * PI2 / 4.0;
  const double k2c = PI4 * (1 - 2 * z2) / 16.0;
  const double k3d = PI6 * (5 - 30 * z2) / 64.0;
  const double k3c = PI4 * (-60 * z2 + 212 * z4) / 16.0;
  const double k3b = PI2 * (135 * z4 - 96 * z6) / 4.0;
  const double k3a = -30 * z6 - 90 * z8;

  double K0 = 0, K1 = 0, K2 = 0, K3 = 0;
  const int maxk = (int)std::ceil(16.0 * z / M_PI);
  for (int k = maxk; k >= 1; --k) {
    const double m = 2.0 * k - 1.0;
    const double m2 = m * m, m4 = m2 * m2, m6 = m4 * m2;
    const double qp = std::pow(q, 8.0 * k);
    K0 = K0 * qp + 1.0;
    K1 = K1 * qp + (k1a + k1b * m2);
    K2 = K2 * qp + (k2a + k2b * m2 + k2c * m4);
    K3 = K3 * qp + (k3a + k3b * m2 + k3c * m4 + k3d * m6);
  }
  K0 *= q * SQRT2PI / z;
  K1 *= q * SQRT2PI / (6 * z4);
  K2 *= q * SQRT2PI / (72 * z7);
  K3 *= q * SQRT2PI / (6480 * z10);

  const double q2 = std::exp(-PI2 / 2.0 / z2);
  double k2x = 0, k3x = 0;
  for (int k = 1; k <= maxk; ++k) {
    const double k2_ = (double)k * k;
    const double qpw = std::pow(q2, k2_);
    k2x += k2_ * qpw;
    const double kspi = M_PI * k;
    const double s3z = std::sqrt(3.0) * z;
    k3x += (s3z + kspi) * (s3z - kspi) * k2_ * qpw;
  }
  K2 += k2x * PI2 * SQRT2PI / (-36 * z3);
  K3 += k3x * PI2 * SQRT2PI / (216 * z6);

  const double sq = std::sqrt(n);
  const double cdf = K0 + K1 / sq + K2 / n + K3 / (n * sq);
  return std::min(1.0, std::max(0.0, 1.0 - cdf));
}

// One-sided Smirnov tail P(D_n^+ >= x), 0 < x < 1, by the Birnbaum-Tingey
// sum x * sum_j C(n,j) (x + j/n)^(j-1) (1 - x - j/n)^(n-j), j <= n(1-x).
// All terms are positive; each is formed in logs, with log C(n,j) carried
// from term to term (three logs and one exp per term, at most n terms).
inline double smirnov_sf(int n, double x) {
  const int jmax = (int)std::floor(n * (1.0 - x));
  double sum = 0.0;
  double log_c = 0.0;  // log C(n, j)
  for (int j = 0; j <= jmax; ++j) {
    if (j > 0) log_c += std::log((double)(n - j + 1) / j);
    const double a = x + (double)j / n;
    const double b = 1.0 - x - (double)j / n;
    if (b <= 0.0) continue;  // j = n (1 - x) exactly: the term is 0
    sum += std::exp(log_c + (j - 1) * std::log(a) + (n - j) * std::log(b));
  }
  return std::min(1.0, std::max(0.0, x * sum));
}

inline void drift_pvals_raw(const int32_t* bh, const float* kd, int nnum,
                            const int32_t* rc, const int32_t* off, int ncat,
                            int64_t n_ref, int64_t n_batch, double* pv) {

  for (int j = 0; j < ncat; ++j) {
    double rsum = 0, bsum = 0;
    int k = 0;
    const int lo = off[j], hi = off[j + 1];
    for (int i = lo; i < hi; ++i) {
      if (rc[i] + bh[i] > 0) { ++k; rsum += rc[i]; bsum += bh[i]; }
    }
    if (k < 2 || rsum == 0 || bsum == 0) { pv[j] = 1.0; continue; }
    const double n = rsum + bsum;
    double stat = 0;
    for (int i = lo; i < hi; ++i) {
      const double tot = (double)rc[i] + bh[i];
      if (tot <= 0) continue;
      const double er = tot * (rsum / n), eb = tot * (bsum / n);
      double dr = std::fabs(rc[i] - er), db = std::fabs(bh[i] - eb);
      if (k == 2) {  // Yates continuity correction on 2x2
        dr = std::max(dr - 0.5, 0.0);
        db = std::max(db - 0.5, 0.0);
      }
      stat += dr * dr / er + db * db / eb;
    }
    pv[j] = chi2_sf_int_dof(stat, k - 1);
  }

  const double en_f = (double)n_ref * (double)n_batch / ((double)n_ref + (double)n_batch);
  const double en = std::nearbyint(en_f);
  // The target is scipy.stats.kstwo.sf(D, en), what ks_2samp(method="asymp")
  // and so models/drift.ks_asymp_pvalue report. Above n = 140 scipy itself
  // (Simard & L'Ecuyer 2011) selects by region, and so does this:
  //   en <= 140: exact MTW;
  //   en D^2 >= 2.2: twice the one-sided Smirnov tail. Below en = 300 it is
  //     evaluated as such (Pelz-Good is 5e-7 off it at en = 141); from 300
  //     on Pelz-Good stands in, measured <= 1.1e-7 from it;
  //   en D^1.5 <= 1.4: Durbin's exact matrix, i.e. MTW (k <= 1.25 en^(1/3)
  //     + 1, a small matrix). Pelz-Good misses it by 3e-6 at en = 141 and
  //     3.4e-7 at en = 300 but < 3e-7 from en = 320, so this stops at 500;
  //   otherwise Pelz-Good, the same series as scipy's.
  // Checked against kstwo.sf to 3e-7 in tests/test_drift_pvals_host.py.
  for (int j = 0; j < nnum; ++j) {
    const double d = (double)kd[j];
    double p;
    if (en <= 140.0) {
      p = mtw_sf((int)en, d);
    } else if (en < 300.0 && d > 0.0 && d < 1.0 && (en * d) * d >= 2.2) {
      p = std::min(1.0, 2.0 * smirnov_sf((int)en, d));
    } else if (en < 500.0 && en * d * std::sqrt(std::max(d, 0.0)) <= 1.4) {
      p = mtw_sf((int)en, d);
    } else {
      p = pelz_good_sf(d, en);
    }
    pv[ncat + j] = p;
  }
}

// ---------------------------------------------------------------------------
// Response serializer: the reference-shaped /score response straight to
// JSON bytes (shortest-round-trip doubles via std::to_chars). Skips the
// Python dict + json.dumps pass on the serving hot path.
// ---------------------------------------------------------------------------

inline void append_double(std::string& out, double v) {
  // JSON has no spelling for these; json.dumps on the dict path writes
  // NaN, Infinity and -Infinity, and so does this (to_chars: nan, inf)
  if (!std::isfinite(v)) {
    out += std::isnan(v) ? "NaN" : (v > 0 ? "Infinity" : "-Infinity");
    return;
  }
  char buf[32];
  auto [p, ec] = std::to_chars(buf, buf + sizeof(buf), v);
  (void)ec;
  // JSON requires a fraction or exponent for floats; Python emits "0.0"
  // style. Keep parity: append ".0" to bare integers.
  bool has_dot = false;
  for (char* c = buf; c < p; ++c)
    if (*c == '.' || *c == 'e' || *c == 'E') { has_dot = true; break; }
  out.append(buf, p);
  if (!has_dot) out += ".0";
}

// The whole /score response: b predictions, b outlier flags (any non-zero
// value is written as 1.0) and one drift score per name, 1 - p formed in
// float32 (reference 02-register cell-9 semantics). Appends to out.
inline void write_response_json(std::string& out, const double* proba,
                                const double* outlier, int64_t b,
                                const double* pv,
                                const std::vector<std::string>& names) {
  out.reserve(out.size() + (size_t)b * 24 + 2048);
  out += "{\"predictions\": [";
  for (int64_t i = 0; i < b; ++i) {
    if (i) out += ", ";
    append_double(out, proba[i]);
  }
  out += "], \"outliers\": [";
  for (int64_t i = 0; i < b; ++i) {
    if (i) out += ", ";
    out += (outlier[i] != 0.0) ? "1.0" : "0.0";
  }
  out += "], \"feature_drift_batch\": {";
  for (size_t j = 0; j < names.size(); ++j) {
    if (j) out += ", ";
    out += '\"';
    out += names[j];
    out += "\": ";
    append_double(out, (double)(1.0f - (float)pv[j]));
  }
  out += "}}";
}
