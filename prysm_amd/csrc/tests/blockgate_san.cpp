// The block gate's rule on the CPU, under ASan+UBSan (plain g++; no GPU code): blockgate_dev.h --
// the text pz_block_gate_kernel compiles -- driven through a sequential form of the kernel's two
// passes over arrays of exactly their sizes, against a straightforward restatement of
// blockchain/service.go:281-318 (the loop over processAttestation, the last error's verdict, the
// loop over calculateBlockVoteCache) and core.go:300-374 (getSignedParentHashes' slice bounds,
// getAttesterIndices' index and walk), which derives parents and committee of every row on its own,
// whatever the checks said.  The checks' statuses come from a restatement of core.go:240-297 here,
// so every status is reached through the scalars that produce it: every status x {open, closed,
// unaccepted} block, the wrap cases of start / end / idx, m in {0, 1, 63, 64, 65}, inverted and
// overlong att_first pairs, blocks of 0..130 rows, and random batches.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../blockgate_dev.h"

using namespace pz;

namespace {

constexpr int32_t kSentinel = 0x5A5A5A5A;

struct Table {  // ShardAndCommitteesForSlots: per array its (shard, committee id, committee size)
  struct Entry { uint64_t shard; uint32_t comm; uint64_t size; };
  std::vector<std::vector<Entry>> arr;
};

struct Chain {
  uint64_t last_justified_slot, last_state_recalc, n_recent;
  Table tab;
};

struct Row {
  uint64_t slot, jslot, shard, m;  // m = len(ObliqueParentHashes)
  uint64_t blen;                   // len(AttesterBitfield)
  bool trailing;                   // a padding bit of the last byte is set
  int32_t rec;                     // the record's decode status
};

struct Block {
  uint64_t slot;
  int32_t top;  // the decoder's top-level status
  uint8_t candidate;
  std::vector<Row> rows;
};

struct Derived {
  enum { kPanic, kError, kFound } what;
  uint32_t comm;
  uint64_t start;
};

// getSignedParentHashes' bounds (core.go:348-360), then getAttesterIndices (core.go:363-374).
Derived derive(const Chain& c, uint64_t bs, const Row& r) {
  const uint64_t start = bs - r.slot, end = bs - r.slot - r.m + 64;
  if (start > end || end > c.n_recent) return {Derived::kPanic, 0, 0};
  const uint64_t idx = r.slot - c.last_state_recalc;
  if (idx >= c.tab.arr.size()) return {Derived::kPanic, 0, 0};
  for (const auto& e : c.tab.arr[idx])
    if (e.shard == r.shard) return {Derived::kFound, e.comm, start};
  return {Derived::kError, 0, 0};
}

// processAttestation's checks (core.go:240-297) -> status, committee, parents_start.
void process_attestation(const Chain& c, uint64_t bs, const Row& r, int32_t* st, uint32_t* comm, uint64_t* ps) {
  *comm = UINT32_MAX, *ps = 0;
  if ((int64_t)r.slot > (int64_t)bs) { *st = PZ_ATT_SLOT_HIGH; return; }
  if ((int64_t)r.slot < (int64_t)bs - 64) { *st = PZ_ATT_SLOT_LOW; return; }
  if (r.jslot != c.last_justified_slot) { *st = PZ_ATT_JUSTIFIED; return; }
  const uint64_t start = bs - r.slot, end = bs - r.slot - r.m + 64;
  if (start > end || end > c.n_recent) { *st = PZ_ERANGE; return; }
  const uint64_t idx = r.slot - c.last_state_recalc;
  if (idx >= c.tab.arr.size()) { *st = PZ_EINDEX; return; }
  *ps = start;
  const Table::Entry* hit = nullptr;
  for (const auto& e : c.tab.arr[idx])
    if (e.shard == r.shard) { hit = &e; break; }
  if (!hit) { *st = PZ_ATT_NO_COMMITTEE; return; }
  *comm = hit->comm;
  if ((hit->size + 7) / 8 != r.blen) { *st = PZ_ATT_BITFIELD_LEN; return; }
  if ((hit->size & 7) && r.trailing) { *st = PZ_ATT_TRAILING_BITS; return; }
  *st = PZ_ATT_PROCESSED;
}

// A batch as the arrays the gate reads, each of exactly its size.
struct Arrays {
  std::vector<uint64_t> att_first, slot, block_slot, n_oblique, shard, arr_offs, arr_shard, pstart;
  std::vector<int32_t> block_status, rec_status, status, vote;
  std::vector<uint8_t> candidate, report, take;
  std::vector<uint32_t> arr_comm, comm;
  uint32_t flags = 0;
  pz_block_gate_batch g{};
};

void build(const Chain& c, const std::vector<Block>& blocks, Arrays* a) {
  a->att_first.assign(1, 0);
  for (const Block& b : blocks) {
    a->block_status.push_back(b.top);
    a->candidate.push_back(b.candidate);
    for (const Row& r : b.rows) {
      int32_t st;
      uint32_t comm;
      uint64_t ps;
      process_attestation(c, b.slot, r, &st, &comm, &ps);
      a->slot.push_back(r.slot), a->block_slot.push_back(b.slot), a->n_oblique.push_back(r.m), a->shard.push_back(r.shard);
      a->rec_status.push_back(r.rec), a->status.push_back(st), a->comm.push_back(comm), a->pstart.push_back(ps);
    }
    a->att_first.push_back(a->slot.size());
  }
  a->arr_offs.assign(1, 0);
  for (const auto& arr : c.tab.arr) {
    for (const auto& e : arr) a->arr_shard.push_back(e.shard), a->arr_comm.push_back(e.comm);
    a->arr_offs.push_back(a->arr_shard.size());
  }
  const size_t n = a->slot.size();
  a->vote.assign(n, kSentinel), a->take.assign(n, 0xEE), a->report.assign(blocks.size(), 0xEE);
  a->arr_shard.shrink_to_fit(), a->arr_comm.shrink_to_fit();
}

void view(const Chain& c, Arrays* a, bool with_rec, bool with_cand) {
  pz_block_gate_batch& g = a->g;
  g = pz_block_gate_batch{};
  g.nblocks = a->block_status.size();
  g.att_first = a->att_first.data(), g.block_status = a->block_status.data();
  g.rec_status = with_rec ? a->rec_status.data() : nullptr;
  g.candidate = with_cand ? a->candidate.data() : nullptr;
  g.chk.natt = a->slot.size();
  g.chk.slot = a->slot.data(), g.chk.block_slot = a->block_slot.data(), g.chk.n_oblique = a->n_oblique.data();
  g.chk.shard_id = a->shard.data();
  g.chk.last_justified_slot = c.last_justified_slot, g.chk.last_state_recalc = c.last_state_recalc, g.chk.n_recent = c.n_recent;
  g.chk.narr = c.tab.arr.size();
  g.chk.arr_offs = a->arr_offs.data(), g.chk.arr_shard = a->arr_shard.data(), g.chk.arr_comm = a->arr_comm.data();
  g.chk.status = a->status.data(), g.chk.committee = a->comm.data(), g.chk.parents_start = a->pstart.data();
  g.report = a->report.data(), g.vote_status = a->vote.data(), g.pend_take = a->take.data(), g.flags = &a->flags;
}

// pz_block_gate_kernel, a block at a time (its waves share nothing): pass 1's reductions as plain
// sums over the rows, pass 2 a row at a time.
void run_gate(const pz_block_gate_batch& g) {
  for (uint64_t b = 0; b < g.nblocks; ++b) {
    const uint64_t f0 = g.att_first[b], f1 = g.att_first[b + 1];
    if (!bg_span_ok(f0, f1, g.chk.natt)) {
      g.report[b] = kBgRejected;
      continue;
    }
    const uint64_t n = f1 - f0;
    uint64_t nproc = 0;
    bool bad = false, panicked = false;
    for (uint64_t i = f0; i < f1; ++i) {
      bad = bad || (g.rec_status && g.rec_status[i] != PZ_OK);
      nproc += g.chk.status[i] == PZ_ATT_PROCESSED;
      panicked = panicked || bg_check_panicked(g.chk.status[i]);
    }
    const bool accepted = g.block_status[b] == PZ_OK && !bad;
    const uint8_t report = bg_report(accepted, n, nproc, n ? g.chk.status[f1 - 1] : -1);
    const bool open = report != kBgRejected;
    bool panic = accepted && panicked;
    for (uint64_t i = f0; i < f1; ++i) {
      const BgRow r = bg_row(g.chk, i, open);
      panic = panic || r.panic;
      g.vote_status[i] = r.vote_status;
      if (g.pend_take) g.pend_take[i] = bg_pend_take(g.chk.status[i], open, g.candidate, b) ? 1 : 0;
      if (r.rederived) g.chk.committee[i] = r.committee, g.chk.parents_start[i] = r.parents_start;
    }
    g.report[b] = report;
    if (panic) *g.flags |= kBgPanic;
  }
}

struct Counts {
  uint64_t blocks = 0, rows = 0, rederived = 0, panics = 0, batches = 0;
  uint64_t seen[3][16] = {};  // [unaccepted / closed / open][status code]
};

int code_of(int32_t st) { return st >= 0 ? st : st == PZ_ERANGE ? 8 : st == PZ_EINDEX ? 9 : 10; }

#define EXPECT(cond, ...)                                  \
  do {                                                     \
    if (!(cond)) {                                         \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__);     \
      std::printf(__VA_ARGS__);                            \
      std::printf("\n");                                   \
      std::exit(1);                                        \
    }                                                      \
  } while (0)

// service.go:281-318 over one batch, and the comparison with what the gate wrote.
void check(const Chain& c, const std::vector<Block>& blocks, bool with_rec, bool with_cand, Counts* k) {
  Arrays a;
  build(c, blocks, &a);
  view(c, &a, with_rec, with_cand);
  const std::vector<int32_t> status = a.status;
  const std::vector<uint32_t> comm0 = a.comm;
  const std::vector<uint64_t> ps0 = a.pstart;
  run_gate(a.g);
  bool panic = false;
  uint64_t i = 0;
  for (size_t b = 0; b < blocks.size(); ++b) {
    const Block& blk = blocks[b];
    bool accepted = blk.top == PZ_OK;
    for (const Row& r : blk.rows) accepted = accepted && (!with_rec || r.rec == PZ_OK);
    // the loop over processAttestation (service.go:281-301)
    bool can = false, all = true;
    std::vector<uint64_t> processed;
    for (size_t j = 0; j < blk.rows.size(); ++j) {
      const int32_t st = status[i + j];
      if (accepted && (st == PZ_ERANGE || st == PZ_EINDEX)) panic = true;  // it panicked (core.go:353, :367)
      can = st == PZ_ATT_PROCESSED;
      all = all && can;
      if (can) processed.push_back(i + j);
    }
    const bool open = accepted && can;  // service.go:304-306 (no attestation: canProcessAttestations stays false)
    EXPECT(a.report[b] == (open ? (all ? 1 : 2) : 0), "report of block %zu: %d", b, a.report[b]);
    for (size_t j = 0; j < blk.rows.size(); ++j) {
      const uint64_t at = i + j;
      const int32_t st = status[at];
      k->seen[!accepted ? 0 : open ? 2 : 1][code_of(st)]++;
      int32_t want = st == PZ_ATT_PROCESSED ? PZ_ATT_NOT_PROCESSED : st;
      uint32_t want_comm = comm0[at];
      uint64_t want_ps = ps0[at];
      if (open && !(st == PZ_ERANGE || st == PZ_EINDEX)) {
        // calculateBlockVoteCache (service.go:313-318): derived afresh for every row
        const Derived d = derive(c, blk.slot, blk.rows[j]);
        if (d.what == Derived::kPanic) panic = true;
        if (d.what == Derived::kFound) {
          want = PZ_ATT_PROCESSED, want_comm = d.comm, want_ps = d.start;
          k->rederived += st == PZ_ATT_SLOT_HIGH || st == PZ_ATT_SLOT_LOW || st == PZ_ATT_JUSTIFIED;
        } else if (st == PZ_ATT_PROCESSED) {
          EXPECT(false, "a PROCESSED row the restatement cannot derive");
        }
      }
      EXPECT(a.vote[at] == want, "vote_status of row %llu: %d, want %d (status %d)", (unsigned long long)at, a.vote[at], want, st);
      EXPECT(a.comm[at] == want_comm && a.pstart[at] == want_ps, "committee / parents_start of row %llu", (unsigned long long)at);
      const bool take = open && st == PZ_ATT_PROCESSED && (!with_cand || blk.candidate);
      EXPECT(a.take[at] == (take ? 1 : 0), "pend_take of row %llu", (unsigned long long)at);
    }
    i += blk.rows.size();
    k->blocks++, k->rows += blk.rows.size();
  }
  EXPECT(((a.flags & kBgPanic) != 0) == panic, "panic flag %u, want %d", a.flags, (int)panic);
  EXPECT(a.status == status, "the gate wrote the checks' status");
  k->panics += panic;
  k->batches++;
}

Chain make_chain(std::mt19937_64& rng, uint64_t lsr, uint64_t n_recent, size_t narr) {
  Chain c{7, lsr, n_recent, {}};
  uint32_t id = 0;
  for (size_t a = 0; a < narr; ++a) {
    std::vector<Table::Entry> arr;
    const int ne = 1 + (int)(rng() % 3);
    for (int e = 0; e < ne; ++e) arr.push_back({(uint64_t)(10 * (a % 7) + e), id++, 9 + rng() % 20});
    c.tab.arr.push_back(arr);
  }
  return c;
}

uint64_t size_of(const Chain& c, uint64_t slot, uint64_t shard) {
  const uint64_t idx = slot - c.last_state_recalc;
  if (idx < c.tab.arr.size())
    for (const auto& e : c.tab.arr[idx])
      if (e.shard == shard) return e.size;
  return 0;
}

// A row of block slot bs that processAttestation passes (m obliques).
Row good(const Chain& c, uint64_t slot, uint64_t m = 0) {
  const uint64_t idx = slot - c.last_state_recalc;
  const uint64_t shard = idx < c.tab.arr.size() ? c.tab.arr[idx][0].shard : 0;
  return {slot, c.last_justified_slot, shard, m, (size_of(c, slot, shard) + 7) / 8, false, PZ_OK};
}

}  // namespace

int main() {
  std::mt19937_64 rng(20);
  Counts k;
  // ---- every status, in an open, a closed and an unaccepted block -------------------------
  {
    const Chain c = make_chain(rng, 64, 128, 128);
    const uint64_t bs = 200;  // the window is slots 136..200: arrays 72..136 of 128
    uint64_t S = 150, P = 150;  // P: a slot whose first committee pads its last bitfield byte
    while (size_of(c, P, c.tab.arr[P - 64][0].shard) % 8 == 0) ++P;
    EXPECT(P < 190, "no committee with padding bits");
    std::vector<Row> kinds;
    kinds.push_back(good(c, S));                                   // PROCESSED
    kinds.push_back(good(c, bs + 1));                              // SLOT_HIGH: start wraps, a panic
    kinds.push_back(good(c, 135, 1));                              // SLOT_LOW: start 65, end 128: tallied
    kinds.push_back(good(c, 135, 0));                              // SLOT_LOW: end 129 > 128, a panic
    { Row r = good(c, S); r.jslot = 8; kinds.push_back(r); }       // JUSTIFIED: tallied
    { Row r = good(c, S); r.jslot = 8; r.shard = 999; kinds.push_back(r); }  // JUSTIFIED, no committee
    { Row r = good(c, S); r.jslot = 8; r.m = 65; kinds.push_back(r); }       // JUSTIFIED, start > end
    { Row r = good(c, 195); r.jslot = 8; kinds.push_back(r); }     // JUSTIFIED, idx 131 >= 128
    { Row r = good(c, S); r.shard = 999; kinds.push_back(r); }     // NO_COMMITTEE
    { Row r = good(c, S); r.blen += 1; kinds.push_back(r); }       // BITFIELD_LEN (long)
    { Row r = good(c, S); r.blen -= 1; kinds.push_back(r); }       // BITFIELD_LEN (short)
    { Row r = good(c, P); r.trailing = true; kinds.push_back(r); } // TRAILING_BITS
    kinds.push_back(good(c, S, 65));                               // PZ_ERANGE
    kinds.push_back(good(c, 195));                                 // PZ_EINDEX: idx 131 >= 128
    for (const Row& r : kinds)
      for (int shape = 0; shape < 4; ++shape) {  // open / closed by its last row / bad top level / a bad record
        Block b{bs, shape == 2 ? PZ_EINVAL : PZ_OK, 1, {r, good(c, S + 1)}};
        if (shape == 1) b.rows.push_back([&] { Row x = good(c, S); x.jslot = 9; return x; }());
        if (shape == 3) b.rows[1].rec = PZ_EINVAL;
        for (int rec = 0; rec < 2; ++rec)
          for (int cand = 0; cand < 2; ++cand) {
            b.candidate = (uint8_t)cand;
            check(c, {b}, rec != 0, true, &k);
          }
        check(c, {b}, true, false, &k);
      }
    // lastStateRecalc above the slot: idx = slot - lsr wraps (core.go:367)
    Row r = good(c, S);
    r.slot = 60, r.m = 2;  // bs 126: SLOT_LOW, start 66, end 128; idx = 60 - 64 wraps
    check(c, {Block{126, PZ_OK, 1, {r, good(c, 100)}}}, true, true, &k);
  }
  // ---- m x start x n_recent x narr: the bounds at their edges --------------------------------
  for (uint64_t n_recent : {0ull, 63ull, 64ull, 128ull, 129ull, ~0ull})
    for (uint64_t lsr : {0ull, 64ull, ~0ull - 3})
      for (size_t narr : {(size_t)0, (size_t)1, (size_t)128}) {
        const Chain c = make_chain(rng, lsr, n_recent, narr);
        std::vector<Block> blocks;
        for (uint64_t m : {0ull, 1ull, 63ull, 64ull, 65ull, ~0ull})
          for (uint64_t back : {0ull, 1ull, 64ull, 65ull, 66ull, 129ull, ~0ull, 1ull << 63}) {  // bs - slot
            const uint64_t bs = lsr + 70;
            Row r = good(c, bs - back, m);
            Row j = r;
            j.jslot = c.last_justified_slot + 1;
            blocks.push_back({bs, PZ_OK, 1, {r, j, good(c, bs - 1)}});
          }
        check(c, blocks, true, true, &k);
        for (const Block& b : blocks) check(c, {b}, false, false, &k);
      }
  // ---- block sizes round the wave, empty blocks, empty batches ---------------------------------
  {
    const Chain c = make_chain(rng, 0, 128, 128);
    std::vector<Block> blocks;
    for (size_t n : {0, 1, 2, 63, 64, 65, 130}) {
      Block b{70, PZ_OK, (uint8_t)(n & 1), {}};
      for (size_t j = 0; j < n; ++j) {
        Row r = good(c, 6 + rng() % 64);
        if (rng() % 4 == 0) r.jslot = 9;
        b.rows.push_back(r);
      }
      blocks.push_back(b);
    }
    check(c, blocks, true, true, &k);
    check(c, {}, true, true, &k);
    check(c, {Block{70, PZ_OK, 1, {}}}, false, false, &k);
  }
  // ---- att_first pairs that name no rows ---------------------------------------------------------
  {
    const Chain c = make_chain(rng, 0, 128, 128);
    std::vector<Block> blocks(3, Block{70, PZ_OK, 1, {good(c, 10), good(c, 11)}});
    for (int which = 0; which < 2; ++which) {
      Arrays a;
      build(c, blocks, &a);
      if (which == 0) a.att_first = {0, 5, 3, 6};  // block 1 inverted; block 0 runs to 5, block 2 is rows 3..6
      else a.att_first = {0, 2, 9, 6};             // block 1 past natt, block 2 inverted
      view(c, &a, true, true);
      run_gate(a.g);
      EXPECT(a.flags == 0, "flags");
      if (which == 0) {
        EXPECT(a.report[0] == 1 && a.report[1] == 0 && a.report[2] == 1, "reports with an inverted pair");
        for (int i = 0; i < 6; ++i) EXPECT(a.vote[i] == PZ_ATT_PROCESSED, "row %d", i);
      } else {
        EXPECT(a.report[0] == 1 && a.report[1] == 0 && a.report[2] == 0, "reports with an overlong pair");
        for (int i = 2; i < 6; ++i) EXPECT(a.vote[i] == kSentinel && a.take[i] == 0xEE, "row %d was written", i);
      }
      k.batches++;
    }
  }
  // ---- random batches ----------------------------------------------------------------------------
  auto pick = [&](std::vector<uint64_t> v) { return v[rng() % v.size()]; };
  for (int it = 0; it < 400; ++it) {
    const uint64_t lsr = (rng() % 3) * 64;
    const Chain c = make_chain(rng, lsr, pick({64, 100, 128, 200}), (size_t)pick({64, 128, 130}));
    std::vector<Block> blocks;
    const size_t nb = (size_t)pick({1, 3, 63, 64, 65});
    for (size_t b = 0; b < nb; ++b) {
      Block blk{lsr + 60 + rng() % 80, rng() % 9 ? PZ_OK : PZ_EINVAL, (uint8_t)(rng() % 4 != 0), {}};
      const size_t n = rng() % 6 ? rng() % 5 : rng() % 140;
      for (size_t j = 0; j < n; ++j) {
        Row r = good(c, blk.slot - rng() % 60, rng() % 3);
        switch (rng() % 14) {
          case 0: r.slot = blk.slot + 1 + rng() % 3; break;
          case 1: r.slot = blk.slot - 65 - rng() % 3; r.m = rng() % 4; break;
          case 2: r.jslot += 1; break;
          case 3: r.jslot += 1; r.shard = 999; break;
          case 4: r.shard = 999; break;
          case 5: r.blen += 1; break;
          case 6: r.blen -= r.blen ? 1 : 0; break;
          case 7: r.trailing = true; break;
          case 8: if (rng() % 8 == 0) r.m = 65; break;
          case 9: if (rng() % 8 == 0) r.rec = PZ_EINVAL; break;
          default: break;
        }
        blk.rows.push_back(r);
      }
      blocks.push_back(blk);
    }
    check(c, blocks, rng() % 2, rng() % 2, &k);
  }
  // every status was met in an open, a closed and an unaccepted block
  for (int shape = 0; shape < 3; ++shape)
    for (int code : {0, 2, 3, 4, 5, 6, 7, 8, 9}) EXPECT(k.seen[shape][code] > 0, "status code %d never met in block shape %d", code, shape);
  std::printf("ok: %llu batches, %llu blocks, %llu rows, %llu re-derived, %llu panics\n", (unsigned long long)k.batches,
              (unsigned long long)k.blocks, (unsigned long long)k.rows, (unsigned long long)k.rederived,
              (unsigned long long)k.panics);
  return 0;
}
