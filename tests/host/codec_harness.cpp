// Stand-alone driver for csrc/host_codec.h: the /score JSON parser, the
// response writer and the drift p-value epilogue, with nothing of torch,
// pybind or HIP, so that it builds with the host sanitizers
// (tests/test_host_codec.py) and nothing has to be loaded into Python.
//
//   codec_harness MODE FILE
//
// FILE is a run of blobs, each a little-endian u32 length and that many
// bytes. Within a blob: str = u32 length + bytes; numbers little-endian.
//
//   parse  blob 0 is the encoder's configuration (u32 ncat, u32 nnum; per
//          categorical column str name, u32 n, n x str vocabulary word; per
//          numeric column str name; str missing category; ncat x i16 default
//          codes; nnum x f32 default nums). Every further blob is a request
//          body. It is copied into a heap block of exactly its length, no
//          terminator, so that a sanitizer sees a read one byte past it.
//          Per body one line: "OK <rows> <hex codes> <hex nums>" (the two
//          arrays' bytes; "-" for none) or "ERR <message>".
//   time   same file; each body is parsed 200 times and the median is
//          printed: "TIME <median ns> <fastest ns> <rows>". Build with -O2
//          and no sanitizer for this mode; to compare two parsers, build it
//          once against each version of the header (-I picks the directory).
//   write  each blob: u32 b, b x f64 predictions, b x f64 outlier flags,
//          u32 nf, nf x str name, nf x f64 p-values (doubles as their bit
//          patterns). Per blob one line, the response JSON.
//   pvals  each blob: i64 n_ref, i64 n_batch, u32 ncat, (ncat + 1) x i32
//          offsets, off[ncat] x i32 reference counts, off[ncat] x i32 batch
//          histogram, u32 nnum, nnum x f32 K-S D. Per blob one line: the
//          ncat + nnum p-values as 16 hex digits each (bit patterns).

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>

#include "host_codec.h"

namespace {

struct Reader {
  const unsigned char* p;
  const unsigned char* end;

  void need(size_t n) const {
    if ((size_t)(end - p) < n) throw std::runtime_error("case file truncated");
  }
  template <typename T>
  T get() {
    need(sizeof(T));
    T v;
    std::memcpy(&v, p, sizeof(T));
    p += sizeof(T);
    return v;
  }
  template <typename T>
  std::vector<T> vec(size_t n) {
    need(n * sizeof(T));
    std::vector<T> v(n);
    if (n) std::memcpy(v.data(), p, n * sizeof(T));
    p += n * sizeof(T);
    return v;
  }
  std::string str() {
    const uint32_t n = get<uint32_t>();
    need(n);
    std::string s((const char*)p, n);
    p += n;
    return s;
  }
  Reader blob() {
    const uint32_t n = get<uint32_t>();
    need(n);
    Reader r{p, p + n};
    p += n;
    return r;
  }
  bool done() const { return p == end; }
};

void put_hex(std::string& out, const void* data, size_t n) {
  static const char* digits = "0123456789abcdef";
  if (n == 0) { out += '-'; return; }
  const unsigned char* b = (const unsigned char*)data;
  for (size_t i = 0; i < n; ++i) {
    out += digits[b[i] >> 4];
    out += digits[b[i] & 15];
  }
}

JsonEncoderState read_config(Reader r) {
  const uint32_t ncat = r.get<uint32_t>(), nnum = r.get<uint32_t>();
  std::vector<std::vector<std::string>> vocab(ncat);
  std::vector<std::string> cats, numn;
  for (uint32_t j = 0; j < ncat; ++j) {
    cats.push_back(r.str());
    const uint32_t n = r.get<uint32_t>();
    for (uint32_t k = 0; k < n; ++k) vocab[j].push_back(r.str());
  }
  for (uint32_t j = 0; j < nnum; ++j) numn.push_back(r.str());
  const std::string missing = r.str();
  std::vector<int16_t> dc = r.vec<int16_t>(ncat);
  std::vector<float> dn = r.vec<float>(nnum);
  if (!r.done()) throw std::runtime_error("configuration blob has trailing bytes");
  return JsonEncoderState(std::move(vocab), cats, numn, missing, std::move(dc),
                          std::move(dn));
}

// The body alone in a heap block of its own length.
std::unique_ptr<char[]> exact_copy(const Reader& body, size_t& n) {
  n = (size_t)(body.end - body.p);
  std::unique_ptr<char[]> block(new char[n]);
  if (n) std::memcpy(block.get(), body.p, n);
  return block;
}

int run_parse(Reader file) {
  const JsonEncoderState st = read_config(file.blob());
  std::string line;
  while (!file.done()) {
    size_t n;
    const std::unique_ptr<char[]> block = exact_copy(file.blob(), n);
    std::vector<int16_t> codes;
    std::vector<float> nums;
    line.clear();
    try {
      const size_t b = parse_records_nogil(st, block.get(), (ptrdiff_t)n, codes, nums);
      if (codes.size() != b * (size_t)st.ncat || nums.size() != b * (size_t)st.nnum)
        throw std::runtime_error("row count and array sizes disagree");
      line = "OK " + std::to_string(b) + " ";
      put_hex(line, codes.data(), codes.size() * sizeof(int16_t));
      line += ' ';
      put_hex(line, nums.data(), nums.size() * sizeof(float));
    } catch (const jsonenc::Error& e) {
      line = "ERR " + e.msg;
    }
    std::puts(line.c_str());
  }
  return 0;
}

int run_time(Reader file) {
  const JsonEncoderState st = read_config(file.blob());
  const int reps = 200;
  while (!file.done()) {
    size_t n;
    const std::unique_ptr<char[]> block = exact_copy(file.blob(), n);
    std::vector<long long> ns(reps);
    size_t rows = 0;
    for (int r = 0; r < reps; ++r) {
      std::vector<int16_t> codes;
      std::vector<float> nums;
      const auto t0 = std::chrono::steady_clock::now();
      rows = parse_records_nogil(st, block.get(), (ptrdiff_t)n, codes, nums);
      const auto t1 = std::chrono::steady_clock::now();
      ns[r] = std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
      if (codes.size() != rows * (size_t)st.ncat) return 1;
    }
    std::sort(ns.begin(), ns.end());
    std::printf("TIME %lld %lld %zu\n", (ns[reps / 2 - 1] + ns[reps / 2]) / 2, ns[0], rows);
  }
  return 0;
}

int run_write(Reader file) {
  while (!file.done()) {
    Reader r = file.blob();
    const uint32_t b = r.get<uint32_t>();
    const std::vector<double> proba = r.vec<double>(b), outl = r.vec<double>(b);
    const uint32_t nf = r.get<uint32_t>();
    std::vector<std::string> names;
    for (uint32_t j = 0; j < nf; ++j) names.push_back(r.str());
    const std::vector<double> pv = r.vec<double>(nf);
    if (!r.done()) throw std::runtime_error("write case has trailing bytes");
    std::string out;
    write_response_json(out, proba.data(), outl.data(), (int64_t)b, pv.data(), names);
    std::puts(out.c_str());
  }
  return 0;
}

int run_pvals(Reader file) {
  std::string line;
  while (!file.done()) {
    Reader r = file.blob();
    const int64_t n_ref = r.get<int64_t>(), n_batch = r.get<int64_t>();
    const uint32_t ncat = r.get<uint32_t>();
    const std::vector<int32_t> off = r.vec<int32_t>((size_t)ncat + 1);
    for (uint32_t j = 0; j < ncat; ++j)
      if (off[j] < 0 || off[j + 1] < off[j]) throw std::runtime_error("bad offsets");
    const std::vector<int32_t> rc = r.vec<int32_t>((size_t)off[ncat]);
    const std::vector<int32_t> bh = r.vec<int32_t>((size_t)off[ncat]);
    const uint32_t nnum = r.get<uint32_t>();
    const std::vector<float> ksd = r.vec<float>(nnum);
    if (!r.done()) throw std::runtime_error("pvals case has trailing bytes");
    std::vector<double> pv((size_t)ncat + nnum);
    drift_pvals_raw(bh.data(), ksd.data(), (int)nnum, rc.data(), off.data(), (int)ncat,
                    n_ref, n_batch, pv.data());
    line.clear();
    for (size_t j = 0; j < pv.size(); ++j) {
      uint64_t bits;
      std::memcpy(&bits, &pv[j], sizeof(bits));
      char buf[20];
      std::snprintf(buf, sizeof(buf), "%s%016llx", j ? " " : "", (unsigned long long)bits);
      line += buf;
    }
    std::puts(line.c_str());
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s parse|time|write|pvals FILE\n", argv[0]);
    return 2;
  }
  const std::string mode = argv[1];
  std::ifstream in(argv[2], std::ios::binary);
  if (!in) {
    std::fprintf(stderr, "cannot open %s\n", argv[2]);
    return 2;
  }
  const std::vector<unsigned char> bytes((std::istreambuf_iterator<char>(in)),
                                         std::istreambuf_iterator<char>());
  const Reader file{bytes.data(), bytes.data() + bytes.size()};
  try {
    if (mode == "parse") return run_parse(file);
    if (mode == "time") return run_time(file);
    if (mode == "write") return run_write(file);
    if (mode == "pvals") return run_pvals(file);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "codec_harness: %s\n", e.what());
    return 3;
  }
  std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
  return 2;
}
