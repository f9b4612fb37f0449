// The rules of the stored CrystallizedState's loader (unwire_state.hip), stated once: where a run
// of length-prefixed records is cut (frame_step), the canonical walks of a ValidatorRecord, of a
// ShardAndCommitteeArray with its ShardAndCommittee entries, of a packed member and of the head
// (fields 1-9 and the crosslink records, messages.proto:59-72, 75-77, 87-90, 122-126), and the
// sequential form of the whole load (frame_host, check_host).  The loader accepts exactly the
// canonical encoding, proto3_canon.h's rule: PersistCrystallizedState only ever stores
// proto.Marshal output (blockchain/core.go:170-177).  Plain C++ plus PZ_CANON_FN: the kernels compile
// these texts, prysm_amd/csrc/tests/unwire_state_san.cpp runs them on the CPU under ASan+UBSan.
//
// The offset of a violation is the position of the key byte of the first field that breaks the
// rule, the innermost one; for a run that ends where no header stands, that position.
#pragma once
#include <stdint.h>

#include "proto3_canon.h"

namespace pz {
namespace ustate {

constexpr uint32_t kTileBytes = 4096;   // T: the positions one framing workgroup covers
constexpr uint32_t kEntries = 512;      // E: the offsets at which a chain may enter a tile
constexpr uint32_t kGroupTiles = 64;    // G: the tiles whose tables one workgroup composes
// A record (key, length, body) longer than E could cross a tile's edge and land past the entries
// the tile publishes: a ValidatorRecord body of kRecordLimit bytes or more is PZ_ERANGE.
constexpr uint64_t kRecordLimit = kEntries - 2;  // 1 + 2 + 509 == E
constexpr uint8_t kTagValidator = 0x5a, kTagCommittees = 0x62;  // fields 11 and 12, length-delimited
constexpr uint64_t kNoOffset = ~0ull;

typedef canon::OffsetCursor<false> Cur;

// ---- framing -------------------------------------------------------------------------------------
// The distance from pos to the next header when a canonical record header stands at pos: the tag, a
// minimal varint length, the body inside d[0, end).  0: no header here (stop).
PZ_CANON_FN uint64_t frame_step(const uint8_t* d, uint64_t pos, uint64_t end, uint8_t tag) {
  if (pos >= end || d[pos] != tag) return 0;
  Cur c = Cur::over(d, pos + 1, end);
  const uint64_t len = canon::get_varint(c);
  if (!c.ok || len > c.left()) return 0;
  return c.pos() - pos + len;
}
// The body of the record whose header stands at pos (frame_step(pos) != 0).
PZ_CANON_FN void frame_body(const uint8_t* d, uint64_t pos, uint64_t end, uint64_t* beg, uint64_t* len) {
  Cur c = Cur::over(d, pos + 1, end);
  *len = canon::get_varint(c);
  *beg = c.pos();
}
PZ_CANON_FN bool frame_long(uint64_t step) { return step > kEntries; }

// ---- ValidatorRecord (messages.proto:110-118) ------------------------------------------------------
struct ValRec {
  uint64_t s[8];      // s[f]: field f's value, f = 1, 2, 5, 6, 7
  uint64_t bpos[2];   // fields 3 and 4: position and length
  uint64_t blen[2];
};
// Fields 1, 2, 5, 6, 7 varints, 3 and 4 bytes; zero scalars and empty bytes absent, no unknown
// field.  *err: the offending field's key.
PZ_CANON_FN bool walk_validator(const uint8_t* d, uint64_t beg, uint64_t len, ValRec* r, uint64_t* err) {
  // (locals named one by one and stored by constant index: a record indexed by the field number
  // would live in scratch memory on the device)
  uint64_t s1 = 0, s2 = 0, s5 = 0, s6 = 0, s7 = 0, p3 = 0, n3 = 0, p4 = 0, n4 = 0;
  Cur c = Cur::over(d, beg, beg + len);
  uint64_t good = beg;
  const bool ok = canon::walk_fields(c, 7, 0xe6, 0, [&](uint32_t f, uint64_t q, uint64_t x) {
    if ((f == 3 || f == 4) && !x) return false;
    if (f == 1) s1 = x;
    else if (f == 2) s2 = x;
    else if (f == 3) p3 = q, n3 = x;
    else if (f == 4) p4 = q, n4 = x;
    else if (f == 5) s5 = x;
    else if (f == 6) s6 = x;
    else s7 = x;
    good = c.pos();
    return true;
  });
  r->s[0] = r->s[3] = r->s[4] = 0;
  r->s[1] = s1, r->s[2] = s2, r->s[5] = s5, r->s[6] = s6, r->s[7] = s7;
  r->bpos[0] = p3, r->blen[0] = n3, r->bpos[1] = p4, r->blen[1] = n4;
  if (!ok) *err = good;
  return ok;
}

// ---- ShardAndCommitteeArray (messages.proto:75-77, 87-90) ---------------------------------------------
// The array's body d[beg, beg + len): a run of field 1, each a ShardAndCommittee -- shard_id (field 1,
// a varint, absent when 0), committee (field 2, packed: never empty, its last byte ends a varint).
// entry(pos, shard, packed_pos, packed_len) for each, pos the entry's header.  The elements of a packed
// field are judged one by one by member_at.
template <class V>
PZ_CANON_FN bool walk_committee_array(const uint8_t* d, uint64_t beg, uint64_t len, V&& entry, uint64_t* err) {
  Cur c = Cur::over(d, beg, beg + len);
  uint64_t good = beg, inner = kNoOffset;
  const bool ok = canon::walk_fields(c, 1, 0, 1, [&](uint32_t, uint64_t q, uint64_t x) {
    Cur e = Cur::over(d, q, q + x);
    uint64_t egood = q, shard = 0, ppos = 0, plen = 0;
    const bool eok = canon::walk_fields(e, 2, 0x2, 0, [&](uint32_t f, uint64_t q2, uint64_t x2) {
      if (f == 1) {
        shard = x2;
      } else {
        if (!x2 || (d[q2 + x2 - 1] & 0x80)) return false;
        ppos = q2, plen = x2;
      }
      egood = e.pos();
      return true;
    });
    if (!eok) {
      inner = egood;
      return false;
    }
    if (!entry(good, shard, ppos, plen)) return false;
    good = c.pos();
    return true;
  });
  if (!ok) *err = inner != kNoOffset ? inner : good;
  return ok;
}

// The packed element that ends at the byte d[last] (top bit clear) of a packed field that begins at
// pbeg: read back from its last byte.  False when it is not a minimal varint of a u32: six bytes or
// more, a 5-byte one above 2^32 - 1, a last byte of 0 behind others.  *first: where it begins.
PZ_CANON_FN bool member_at(const uint8_t* d, uint64_t pbeg, uint64_t last, uint32_t* value, uint64_t* first) {
  uint64_t b = last;
  while (b > pbeg && last - b < 5 && (d[b - 1] & 0x80)) --b;
  *first = b;
  const uint64_t n = last - b + 1;
  if (n > 5) {  // (the element begins further back still: its true first byte)
    while (b > pbeg && (d[b - 1] & 0x80)) --b;
    *first = b;
    return false;
  }
  uint64_t x = 0;
  for (uint64_t k = 0; k < n; ++k) x |= (uint64_t)(d[b + k] & 0x7f) << (7 * k);
  if ((n > 1 && d[last] == 0) || x > 0xffffffffull) return false;
  *value = (uint32_t)x;
  return true;
}

// ---- the head: fields 1-9 and the crosslink records (field 10) ---------------------------------------
struct Head {
  uint64_t f[10];      // f[k]: field k's value, k = 1-7 and 9
  uint64_t seed_pos, seed_len;
  uint64_t nrec;
  uint64_t body_beg;   // the first byte behind field 10
};
// record(index, dynasty, hash_pos, hash_len, slot) for every crosslink record.  Stops in front of the
// first field-11 or field-12 key, or at the end.  A dynasty_seed above 64 bytes does not fit
// pz_cstate_rest and is refused like a violation.
template <class V>
PZ_CANON_FN bool walk_head(const uint8_t* d, uint64_t len, Head* h, V&& record, uint64_t* err) {
  for (int k = 0; k < 10; ++k) h->f[k] = 0;
  h->seed_pos = h->seed_len = h->nrec = 0;
  Cur c = Cur::over(d, 0, len);
  uint32_t prev = 0;
  while (c.more() && d[c.pos()] != kTagValidator && d[c.pos()] != kTagCommittees) {
    const uint64_t at = c.pos();
    *err = at;
    const uint64_t k = canon::get_varint(c);
    const uint64_t f = k >> 3;
    if (!c.ok || f == 0 || f > 10) return false;
    const bool var = f != 8 && f != 10;
    if ((k & 7) != (var ? 0u : 2u) || f < prev || (f == prev && f != 10)) return false;
    prev = (uint32_t)f;
    const uint64_t x = canon::get_varint(c);
    uint64_t q = 0;
    if (!c.ok || (var ? !x : !canon::get_span(c, x, &q))) return false;
    if (var) {
      h->f[f] = x;
    } else if (f == 8) {
      if (!x || x > 64) return false;
      h->seed_pos = q, h->seed_len = x;
    } else {
      Cur r = Cur::over(d, q, q + x);
      uint64_t good = q, dynasty = 0, slot = 0, hpos = 0, hlen = 0;
      const bool ok = canon::walk_fields(r, 3, 0xa, 0, [&](uint32_t rf, uint64_t q2, uint64_t x2) {
        if (rf == 1) dynasty = x2;
        else if (rf == 3) slot = x2;
        else if (!x2) return false;
        else hpos = q2, hlen = x2;
        good = r.pos();
        return true;
      });
      if (!ok) {
        *err = good;
        return false;
      }
      if (!record(h->nrec, dynasty, hpos, hlen, slot)) return false;
      ++h->nrec;
    }
  }
  h->body_beg = c.pos();
  return true;
}

// ---- the sequential form ------------------------------------------------------------------------------
struct Framed {
  int status;          // 0, or the negative code
  uint64_t off;        // the violation, with a status
  uint64_t nval, val_end;   // the records of field 11 and where their run ends
  uint64_t narr, f12_end;   // the arrays of field 12 (f12_end == len when status is 0)
};
constexpr int kUsEinval = -6, kUsErange = -7;  // PZ_EINVAL, PZ_ERANGE

// The plain walk over frame_step from body_beg: the chain of field-11 headers, then the one of
// field 12's top-level arrays, which must end at len.  The CPU check's framing, and what the
// framing kernels are measured against.
inline Framed frame_host(const uint8_t* d, uint64_t len, uint64_t body_beg) {
  Framed r = {0, 0, 0, 0, 0, 0};
  uint64_t p = body_beg;
  for (uint64_t s; (s = frame_step(d, p, len, kTagValidator)) != 0; p += s, ++r.nval)
    if (frame_long(s)) {
      r.status = kUsErange, r.off = p;
      return r;
    }
  r.val_end = p;
  for (uint64_t s; (s = frame_step(d, p, len, kTagCommittees)) != 0; p += s) ++r.narr;
  r.f12_end = p;
  if (p != len) r.status = kUsEinval, r.off = p;
  return r;
}

// The whole verdict of a stored state: the head, the framing, then every record and every entry in
// order, then every member.  What pz_cstate_head, pz_dev_cstate_frame and pz_dev_cstate_decode report
// between them, in that order.
struct Verdict {
  int status;
  uint64_t off, nval, narr, nentries, nmembers;
};
inline Verdict check_host(const uint8_t* d, uint64_t len) {
  Verdict v = {0, 0, 0, 0, 0, 0};
  Head h;
  uint64_t err = 0;
  if (!walk_head(d, len, &h, [](uint64_t, uint64_t, uint64_t, uint64_t, uint64_t) { return true; }, &err)) {
    v.status = kUsEinval, v.off = err;
    return v;
  }
  const Framed fr = frame_host(d, len, h.body_beg);
  v.nval = fr.nval, v.narr = fr.narr;
  if (fr.status) {
    v.status = fr.status, v.off = fr.off;
    return v;
  }
  uint64_t p = h.body_beg;
  for (uint64_t i = 0; i < fr.nval; ++i) {
    uint64_t beg, blen;
    frame_body(d, p, len, &beg, &blen);
    ValRec rec;
    if (!walk_validator(d, beg, blen, &rec, &err)) {
      v.status = kUsEinval, v.off = err;
      return v;
    }
    p = beg + blen;
  }
  for (uint64_t a = 0; a < fr.narr; ++a) {
    uint64_t beg, blen;
    frame_body(d, p, len, &beg, &blen);
    const bool ok = walk_committee_array(d, beg, blen, [&](uint64_t, uint64_t, uint64_t, uint64_t) {
      ++v.nentries;
      return true;
    }, &err);
    if (!ok) {
      v.status = kUsEinval, v.off = err;
      return v;
    }
    p = beg + blen;
  }
  p = fr.val_end;
  uint64_t first_bad = kNoOffset;
  for (uint64_t a = 0; a < fr.narr; ++a) {
    uint64_t beg, blen;
    frame_body(d, p, len, &beg, &blen);
    (void)walk_committee_array(d, beg, blen, [&](uint64_t, uint64_t, uint64_t ppos, uint64_t plen) {
      for (uint64_t k = ppos; k < ppos + plen; ++k) {
        if (d[k] & 0x80) continue;
        uint32_t x;
        uint64_t first;
        ++v.nmembers;
        if (!member_at(d, ppos, k, &x, &first) && first < first_bad) first_bad = first;
      }
      return true;
    }, &err);
    p = beg + blen;
  }
  if (first_bad != kNoOffset) v.status = kUsEinval, v.off = first_bad;
  return v;
}

}  // namespace ustate
}  // namespace pz
