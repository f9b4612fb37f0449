// Host-only sanitizer driver for the stored CrystallizedState's loader rules (unwire_state_dev.h):
// the ASan+UBSan build (Makefile target san_unwire_state) runs check_host -- the head walk,
// frame_host, every record's and every array's canonical walk, every packed member -- over each
// entry of a corpus file (argv[1], written by tests/test_unwire_state.py) and compares the verdict
// with the one the file expects; then the same walk, without an expected verdict, over mutants of
// every entry (each byte changed, each prefix), where only the sanitizers judge.  Every input lies
// in a heap block of exactly its length, so a read one byte past either end is reported.  With a
// second argument the verdicts are written there, a line per entry.  Exit status 0 = clean.
//
// The file: entries of {expected status i8, expected offset u64 (all ones: not checked), length u32,
// the bytes}, little-endian.
#include <cstdio>
#include <memory>
#include <vector>

#include "../unwire_state_dev.h"

namespace {

using Bytes = std::vector<uint8_t>;
using namespace pz::ustate;

Verdict judge(const Bytes& in) {
  const size_t n = in.size();
  std::unique_ptr<uint8_t[]> heap(new uint8_t[n ? n : 1]);  // (exactly the input: no slack either side)
  if (n) std::memcpy(heap.get(), in.data(), n);
  return check_host(heap.get(), n);
}

uint64_t le(const uint8_t* p, int bytes) {
  uint64_t x = 0;
  for (int k = 0; k < bytes; ++k) x |= (uint64_t)p[k] << (8 * k);
  return x;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s corpus [verdicts]\n", argv[0]);
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  Bytes file;
  for (uint8_t buf[65536]; size_t got = std::fread(buf, 1, sizeof buf, f);) file.insert(file.end(), buf, buf + got);
  std::fclose(f);
  FILE* out = argc > 2 ? std::fopen(argv[2], "w") : nullptr;
  size_t cases = 0, mutants = 0, bad = 0;
  for (size_t at = 0; at + 13 <= file.size();) {
    const int want = (int8_t)file[at];
    const uint64_t want_off = le(&file[at + 1], 8), n = le(&file[at + 9], 4);
    at += 13;
    if (at + n > file.size()) {
      std::fprintf(stderr, "corpus entry %zu is cut\n", cases);
      return 2;
    }
    const Bytes in(file.begin() + at, file.begin() + at + n);
    at += n;
    const Verdict v = judge(in);
    if (out)
      std::fprintf(out, "%d %llu %llu %llu %llu %llu\n", v.status, (unsigned long long)v.off, (unsigned long long)v.nval,
                   (unsigned long long)v.narr, (unsigned long long)v.nentries, (unsigned long long)v.nmembers);
    if (v.status != want || (v.status && want_off != kNoOffset && v.off != want_off)) {
      std::fprintf(stderr, "entry %zu: verdict %d at %llu, expected %d at %llu\n", cases, v.status, (unsigned long long)v.off, want,
                   (unsigned long long)want_off);
      ++bad;
    }
    ++cases;
    if (n > 4096) continue;  // (the long entries are walked once)
    for (size_t k = 0; k < n; ++k) {
      Bytes m = in;
      m[k] ^= (uint8_t)(1u << (k % 8));
      (void)judge(m);
      m[k] = 0xff;
      (void)judge(m);
      (void)judge(Bytes(in.begin(), in.begin() + k));
      mutants += 3;
    }
  }
  if (out) std::fclose(out);
  if (bad) return 1;
  std::printf("ok: %zu cases, %zu mutants\n", cases, mutants);
  return 0;
}
