// The attestation store's rule and its list-entry writer (../blockstore_dev.h) on the CPU, under
// ASan+UBSan: a sequential form of pz_dev_block_store_select (flag, tile sums, tile bases, the write
// and the per-block ranks, tile by tile as the kernels take them) and of the dword writer, over
// buffers of exactly the stated sizes (heap vectors: a byte past any of them is an ASan error),
// against a vector-of-records model of blockchain/service.go:281-301.  No GPU code is involved.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../blockstore_dev.h"

using namespace pz;

namespace {

constexpr uint64_t kTile = 256;  // tile_scan.h's

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

struct Rec {  // one attestation of a received block, as the reference's loop sees it
  bool processed;  // processAttestation returned nil
  bool canonical;  // its record decoded
  uint64_t beg, end;
};
struct Block {
  bool decoded, parent_ok;
  std::vector<Rec> atts;
};

struct Cols {
  std::vector<uint64_t> att_first, att_beg, att_end;
  std::vector<int32_t> block_status, att_status, rec_status;
  std::vector<uint8_t> parent_ok;
  std::vector<uint32_t> att_block;
};

Cols columns(const std::vector<Block>& blocks) {
  Cols c;
  c.att_first.push_back(0);
  for (size_t j = 0; j < blocks.size(); ++j) {
    const Block& b = blocks[j];
    bool ok = b.decoded;
    for (const Rec& r : b.atts) {
      ok = ok && r.canonical;
      c.att_block.push_back((uint32_t)j);
      c.att_status.push_back(!r.canonical ? PZ_EINVAL : r.processed ? PZ_ATT_PROCESSED : PZ_ATT_SLOT_HIGH);
      c.rec_status.push_back(r.canonical ? PZ_OK : PZ_EINVAL);
      c.att_beg.push_back(r.beg), c.att_end.push_back(r.end);
    }
    c.block_status.push_back(ok ? PZ_OK : PZ_EINVAL);  // folded: a bad record refuses its block
    c.parent_ok.push_back(b.parent_ok);
    c.att_first.push_back(c.att_block.size());
  }
  return c;
}

struct Out {
  std::vector<uint32_t> rows;
  std::vector<uint64_t> span, first;
  uint64_t m;
};

// service.go:281-301 block by block: what the loop saves, in the order it saves it.
Out model(const std::vector<Block>& blocks, uint64_t stop) {
  Out o;
  uint64_t r = 0;
  for (size_t j = 0; j < blocks.size(); ++j) {
    o.first.push_back(o.rows.size());
    const Block& b = blocks[j];
    bool whole = b.decoded;
    for (const Rec& a : b.atts) whole = whole && a.canonical;
    for (const Rec& a : b.atts) {
      if (j < stop && whole && b.parent_ok && a.processed) {
        o.rows.push_back((uint32_t)r);
        o.span.push_back(a.beg), o.span.push_back(a.end);
      }
      ++r;
    }
  }
  o.first.push_back(o.rows.size());
  o.m = o.rows.size();
  return o;
}

// The four launches, sequentially; with_rec false passes a NULL rec_status (att_status has it folded in).
Out select(const Cols& c, uint64_t nblocks, uint64_t stop, bool with_rec, uint64_t room) {
  const uint64_t natt = c.att_block.size(), ntiles = (natt + kTile - 1) / kTile;
  const int32_t* rec = with_rec ? c.rec_status.data() : nullptr;
  auto flag = [&](uint64_t r) {
    return r < natt && bs_row_saved(r, nblocks, stop, c.att_block.data(), c.block_status.data(), c.parent_ok.data(), c.att_status.data(), rec);
  };
  std::vector<uint64_t> tiles(ntiles);
  for (uint64_t t = 0; t < ntiles; ++t)  // size
    for (uint64_t l = 0; l < kTile; ++l) tiles[t] += flag(t * kTile + l);
  uint64_t total = 0;
  for (uint64_t t = 0; t < ntiles; ++t) {  // scan
    const uint64_t s = tiles[t];
    tiles[t] = total, total += s;
  }
  Out o;
  o.rows.assign(room, 0xA5A5A5A5u), o.span.assign(2 * room, 0xA5A5), o.first.assign(nblocks + 1, 0xA5A5);
  std::vector<uint32_t> rank(natt + 1);
  for (uint64_t t = 0; t < ntiles; ++t) {  // write
    uint64_t ex = 0;
    for (uint64_t l = 0; l < kTile; ++l) {
      const uint64_t r = t * kTile + l, at = tiles[t] + ex;
      if (r < natt) {
        rank[r] = (uint32_t)at;
        if (flag(r)) o.rows[at] = (uint32_t)r, o.span[2 * at] = c.att_beg[r], o.span[2 * at + 1] = c.att_end[r];
      }
      ex += flag(r);
    }
  }
  rank[natt] = (uint32_t)total, o.m = total;
  for (uint64_t j = 0; j <= nblocks; ++j) o.first[j] = bs_first(rank.data(), c.att_first[j], natt);  // first
  return o;
}

std::vector<Block> make_blocks(std::mt19937_64& rng, uint64_t natt, int mode) {
  // mode 0: random statuses; 1: every row saved; 2: none (no parent); blocks of 0 rows at the front,
  // in the middle and at the end
  std::vector<Block> blocks;
  uint64_t left = natt, at = 0;
  blocks.push_back(Block{true, true, {}});
  while (left) {
    Block b{mode ? true : rng() % 8 != 0, mode == 1 ? true : mode == 2 ? false : rng() % 6 != 0, {}};
    const uint64_t k = std::min<uint64_t>(left, rng() % 5);
    for (uint64_t i = 0; i < k; ++i) {
      const uint64_t len = rng() % 300;
      b.atts.push_back(Rec{mode == 1 || rng() % 3 != 0, mode ? true : rng() % 40 != 0, at, at + len});
      at += len;
    }
    left -= k;
    blocks.push_back(b);
  }
  blocks.push_back(Block{true, true, {}});
  return blocks;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20241);
  uint64_t runs = 0, saved = 0, entries = 0;
  for (uint64_t natt : {0ull, 1ull, 255ull, 256ull, 257ull, 513ull})
    for (int mode = 0; mode < 3; ++mode) {
      const std::vector<Block> blocks = make_blocks(rng, natt, mode);
      const Cols c = columns(blocks);
      const uint64_t nb = blocks.size();
      CHECK(c.att_block.size() == natt);
      for (uint64_t stop : {uint64_t(0), nb / 2, nb})
        for (int with_rec = 0; with_rec < 2; ++with_rec) {
          const Out want = model(blocks, stop);
          const Out got = select(c, nb, stop, with_rec, natt);
          CHECK(got.m == want.m && got.first == want.first);
          for (uint64_t i = 0; i < natt; ++i) {  // the m saved rows, then untouched room
            CHECK(got.rows[i] == (i < want.m ? want.rows[i] : 0xA5A5A5A5u));
            CHECK(got.span[2 * i] == (i < want.m ? want.span[2 * i] : 0xA5A5));
            CHECK(got.span[2 * i + 1] == (i < want.m ? want.span[2 * i + 1] : 0xA5A5));
          }
          if (mode == 1 && stop == nb) CHECK(got.m == natt);
          if (mode == 2 || stop == 0) CHECK(got.m == 0);
          ++runs, saved += got.m;
        }
      // a row that names no block of the run is never saved
      if (natt) {
        Cols bad = c;
        for (uint32_t& b : bad.att_block) b = (uint32_t)nb;
        CHECK(select(bad, nb, nb, 1, natt).m == 0);
      }
    }
  // the dword writer: hash[m][32] exactly, lists of exactly 34 m bytes
  for (uint64_t m : {0ull, 1ull, 2ull, 3ull, 255ull, 256ull, 257ull, 513ull}) {
    std::vector<uint8_t> hash(32 * m), lists(34 * m, 0xEE), want;
    for (uint8_t& b : hash) b = (uint8_t)rng();
    for (uint64_t i = 0; i < m; ++i) {
      want.push_back(0x0a), want.push_back(0x20);
      want.insert(want.end(), hash.begin() + 32 * i, hash.begin() + 32 * i + 32);
    }
    CHECK(bs_list_bytes(m) == want.size() && bs_list_dwords(m) == (want.size() + 3) / 4);
    for (uint64_t d = 0; d < bs_list_dwords(m); ++d) {
      const uint32_t v = bs_list_dword(hash.data(), d);
      if (bs_list_whole(d, m)) {
        std::memcpy(lists.data() + 4 * d, &v, 4);
      } else {  // the last dword of an odd m: a halfword
        const uint16_t h = (uint16_t)v;
        CHECK(d + 1 == bs_list_dwords(m) && m % 2 == 1);
        std::memcpy(lists.data() + 4 * d, &h, 2);
      }
    }
    CHECK(lists == want);
    entries += m;
  }
  std::printf("ok: %llu selects, %llu rows saved, %llu list entries\n", (unsigned long long)runs, (unsigned long long)saved,
              (unsigned long long)entries);
  return 0;
}
