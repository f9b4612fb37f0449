// Host-only sanitizer driver for the canonical-form rule (proto3_canon.h): the ASan+UBSan build
// (Makefile target san) walks every entry of a corpus file (argv[1], written by
// tests/test_host_sanitizers.py from tests/canon_corpus.py) with the pointer cursor and with the
// offset cursor, windowed and per byte, and checks that the three walks make the same visitor
// calls and reach the verdict the file expects; then the same agreement, without an expected
// verdict, on mutants of the canonical entries.  Every input lies in a heap block of exactly its
// length, so a read one byte past either end is reported.  Exit status 0 = clean and consistent.
//
// The file: entries of {kind u8 (0: an AttestationRecord, 1: a BeaconBlock whose record spans
// are walked as records), expected verdict u8, length u32 little-endian, the bytes}.
#include <cstdio>
#include <memory>
#include <vector>

#include "../proto3_canon.h"

namespace {

using Bytes = std::vector<uint8_t>;
using namespace pz::canon;

// Appends every visitor call to a trace.
struct Recorder {
  std::vector<uint64_t> t;
  uint64_t first[2] = {0, 0};  // the first top-level bytes field: position and length
  bool nested = false;
  bool scalar(uint32_t f, uint64_t v) { return put({1, f, v}); }
  bool bytes(uint32_t f, uint64_t q, uint64_t len) {
    if (!nested && !first[1]) first[0] = q, first[1] = len;
    return put({2, f, q, len});
  }
  bool oblique(uint64_t q, uint64_t len) { return put({3, q, len}); }
  bool sig(uint64_t x) { return put({4, x}); }
  bool timestamp(int64_t s, int64_t n) { return put({5, (uint64_t)s, (uint64_t)n}); }
  template <class C>
  bool record(const C& c, uint64_t q, uint64_t len) {
    put({6, q, len});
    C s = c.sub(q, len);
    nested = true;
    const bool ok = walk_attestation(s, *this);
    nested = false;
    return ok;
  }
  bool put(std::initializer_list<uint64_t> v) {
    t.insert(t.end(), v);
    return true;
  }
};

template <class C>
bool walk(int kind, C c, Recorder& r) {
  const bool ok = kind ? walk_block(c, r) : walk_attestation(c, r);
  r.t.push_back(ok);
  return ok;
}

// The three walks of one input; -1 when they disagree, else the verdict.  first: receives the
// position and length of the first top-level bytes field (0, 0 without one).
int judge(int kind, const Bytes& in, uint64_t first[2] = nullptr) {
  const size_t n = in.size();
  std::unique_ptr<uint8_t[]> heap(new uint8_t[n ? n : 1]);  // (exactly the input: no slack either side)
  if (n) std::memcpy(heap.get(), in.data(), n);
  const uint8_t* d = heap.get();
  Recorder p, w, b;
  const bool ok = walk(kind, PtrCursor{d, d, d + n, true}, p);
  walk(kind, OffsetCursor<true>::over(d, 0, n), w);
  walk(kind, OffsetCursor<false>::over(d, 0, n), b);
  if (p.t != w.t || p.t != b.t) return -1;
  if (first) std::memcpy(first, p.first, sizeof p.first);
  return ok;
}

void put_len(Bytes& o, uint64_t x) {
  uint8_t tmp[10];
  o.insert(o.end(), tmp, pz::put_varint(tmp, x));
}

}  // namespace

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? std::fopen(argv[1], "rb") : nullptr;
  if (!f) {
    std::puts("FAIL no corpus file");
    return 1;
  }
  std::vector<std::pair<int, Bytes>> canonical;
  size_t entries = 0, mutants = 0;
  uint64_t resized = 0;  // bit L: an input of L bytes was made by resizing a bytes field
  uint8_t hdr[6];
  while (std::fread(hdr, 1, 6, f) == 6) {
    Bytes in(hdr[2] | hdr[3] << 8 | hdr[4] << 16 | (uint32_t)hdr[5] << 24);
    if (in.size() && std::fread(in.data(), 1, in.size(), f) != in.size()) {
      std::puts("FAIL corpus file cut short");
      return 1;
    }
    const int got = judge(hdr[0], in);
    if (got != hdr[1]) {
      std::printf("FAIL entry %zu: %s, the file expects %d\n", entries,
                  got < 0 ? "the cursors disagree" : got ? "accepted" : "rejected", hdr[1]);
      return 1;
    }
    if (got) canonical.emplace_back(hdr[0], in);
    ++entries;
  }
  std::fclose(f);

  uint64_t seed = 0x9E3779B97F4A7C15ull;  // fixed: the same mutants every run
  auto rnd = [&] {
    seed ^= seed << 13;
    seed ^= seed >> 7;
    seed ^= seed << 17;
    return seed;
  };
  auto check = [&](int kind, const Bytes& m, const char* what) {
    ++mutants;
    if (judge(kind, m) >= 0) return true;
    std::printf("FAIL the cursors disagree on a mutant (%s, %zu bytes)\n", what, m.size());
    return false;
  };
  // every truncation, and 16 other values for every byte
  auto mutate = [&](int kind, const Bytes& in) {
    for (size_t n = 0; n < in.size(); ++n)
      if (!check(kind, Bytes(in.begin(), in.begin() + n), "truncated")) return false;
    for (size_t i = 0; i < in.size(); ++i)
      for (int k = 0; k < 16; ++k) {
        Bytes m = in;
        m[i] ^= (uint8_t)(1 + rnd() % 255);
        if (!check(kind, m, "one byte changed")) return false;
      }
    return true;
  };
  for (const auto& c : canonical) {
    if (!mutate(c.first, c.second)) return 1;
    // the window's boundaries: the same input with its first bytes field trimmed or extended
    // until the whole is 15, 16, 17, 31, 32 or 33 bytes long; where what follows that field is
    // too long for that, the input is cut after the field (still a whole message)
    uint64_t first[2];
    judge(c.first, c.second, first);
    if (!first[1]) continue;
    const Bytes& in = c.second;
    size_t lp = first[0];  // the length prefix: minimal, so it ends where the bytes begin
    for (--lp; lp > 0 && (in[lp - 1] & 0x80); --lp) {}
    const size_t tail = in.size() - (first[0] + first[1]);
    for (size_t want : {15, 16, 17, 31, 32, 33})
      for (size_t n = 1; n <= want; ++n) {
        Bytes m(in.begin(), in.begin() + lp);
        put_len(m, n);
        for (size_t k = 0; k < n; ++k) m.push_back(in[first[0] + k % first[1]]);
        if (m.size() + tail <= want) m.insert(m.end(), in.end() - tail, in.end());
        if (m.size() != want) continue;
        if (!check(c.first, m, "bytes field resized") || !mutate(c.first, m)) return 1;
        resized |= 1ull << want;
        break;
      }
  }
  if (resized != (1ull << 15 | 1ull << 16 | 1ull << 17 | 1ull << 31 | 1ull << 32 | 1ull << 33)) {
    std::puts("FAIL no canonical entry could be resized to every boundary length");
    return 1;
  }
  if (mutants < 20000) {
    std::printf("FAIL only %zu mutants\n", mutants);
    return 1;
  }
  std::printf("ok %zu corpus entries, %zu mutants\n", entries, mutants);
  return 0;
}
