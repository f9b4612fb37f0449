// The canonical-form rule for serialized BeaconBlocks and AttestationRecords, stated once
// (DESIGN.md §7): an input is accepted only if it is the encoding of its own decoding -- the
// reference hashes proto.Marshal of the DECODED message.  Instead of re-encoding, every rule
// Marshal applies is checked while reading: minimal varints (keys, values, lengths), ascending
// field numbers (a repeated field only repeats in a run), zero scalars and empty singular bytes
// absent, a packed field never empty, no unknown fields.
//
// The walks are templates over a cursor (where the bytes come from: chain.hip's host threads
// use the pointer cursor, unwire.hip's kernels the offset cursor, tests/proto3_canon_san.cpp
// both under ASan and UBSan) and a visitor (what the consumer keeps).  A cursor has more(),
// next() (the next byte, advancing), left(), pos(), advance(len), sub(pos, len) (a cursor over
// a span of the same input) and the failure flag `ok`; a visitor the calls named at the walks,
// each failing the walk by returning false.  Plain C++ outside the device pass.
#pragma once
#include <cstdint>
#include <cstring>

#ifdef __HIP__
#define PZ_CANON_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define PZ_CANON_FN inline
#endif

namespace pz {

// uvarint(x) at p (Go's binary.PutUvarint, proto3's varint); returns the byte after it.
PZ_CANON_FN uint8_t* put_varint(uint8_t* p, uint64_t x) {
  while (x >= 0x80) {
    *p++ = (uint8_t)(x | 0x80);
    x >>= 7;
  }
  *p++ = (uint8_t)x;
  return p;
}

namespace canon {

// a minimal varint (a 10-byte one must end in 0x01: only bit 63 left)
template <class C>
PZ_CANON_FN uint64_t get_varint(C& c) {
  uint64_t x = 0;
  for (int i = 0, s = 0; i < 10; ++i, s += 7) {
    if (!c.more()) break;
    const uint32_t b = c.next();
    x |= (uint64_t)(b & 0x7f) << s;
    if (!(b & 0x80)) {
      if ((i > 0 && b == 0) || (i == 9 && b != 1)) c.ok = false;
      return x;
    }
  }
  c.ok = false;
  return 0;
}

// the bytes a length covers, *q their position (`len > left`: a length of 2^63 never wraps)
template <class C>
PZ_CANON_FN bool get_span(C& c, uint64_t len, uint64_t* q) {
  if (len > c.left()) return c.ok = false;
  *q = c.pos();
  c.advance(len);
  return true;
}

// A message with fields 1..nfields: bit f of `varints` says field f is a varint (the others are
// length-delimited), `rep` is the field that may repeat.  Fails on field 0, an unknown field, a
// wrong wire type, descending order, a repeated singular field and a zero varint (Marshal omits
// it).  field(f, pos, x) for each: x is the varint's value, or the length of the bytes at pos.
template <class C, class F>
PZ_CANON_FN bool walk_fields(C& c, uint32_t nfields, uint32_t varints, uint32_t rep, F&& field) {
  uint32_t prev = 0;
  while (c.more()) {
    const uint64_t k = get_varint(c);
    const uint64_t f = k >> 3;
    const bool var = f <= nfields && ((varints >> f) & 1);
    if (!c.ok || f == 0 || f > nfields || (k & 7) != (var ? 0u : 2u)) return false;
    if (f < prev || (f == prev && f != rep)) return false;
    prev = (uint32_t)f;
    uint64_t q = 0;
    const uint64_t x = get_varint(c);  // (one reader for a value and for a length)
    if (!c.ok || (var ? !x : !get_span(c, x, &q)) || !field(prev, q, x)) return false;
  }
  return true;
}

// Timestamp {int64 seconds = 1; int32 nanos = 2}; an empty message is canonical (a set message
// is emitted).  v.timestamp(seconds, nanos) once, at the end.
template <class C, class V>
PZ_CANON_FN bool walk_timestamp(C& t, V&& v) {
  int64_t seconds = 0, nanos = 0;
  return walk_fields(t, 2, 0x6, 0, [&](uint32_t f, uint64_t, uint64_t x) {
    // int32: Marshal sign-extends the decoded 32-bit value
    if (f == 2 && x != (uint64_t)(int64_t)(int32_t)(uint32_t)x) return false;
    (f == 1 ? seconds : nanos) = (int64_t)x;
    return true;
  }) && v.timestamp(seconds, nanos);
}

// AttestationRecord (messages.pb.go:889-896): 1-3 varint -> v.scalar(f, x); 4-6 bytes, never
// empty (Marshal omits an empty singular bytes field) -> v.bytes(f, pos, len); 7 repeated
// bytes -> v.oblique(pos, len), every element, an empty one too; 8 packed varints, never empty,
// every varint whole and minimal -> v.sig(x) each.
template <class C, class V>
PZ_CANON_FN bool walk_attestation(C& c, V&& v) {
  return walk_fields(c, 8, 0xe, 7, [&](uint32_t f, uint64_t q, uint64_t x) {
    if (f <= 3) return v.scalar(f, x);
    if (f <= 6) return x && v.bytes(f, q, x);
    if (f == 7) return v.oblique(q, x);
    C s = c.sub(q, x);
    while (s.more()) {
      const uint64_t y = get_varint(s);
      if (!s.ok || !v.sig(y)) return false;
    }
    return x != 0;
  });
}

// BeaconBlock, the top level (messages.pb.go:224-232): 1, 3-6 bytes, never empty ->
// v.bytes(f, pos, len); 2 varint -> v.scalar(2, x); 7 Timestamp -> v.timestamp; 8 repeated
// AttestationRecord -> v.record(c, pos, len) with the block's cursor (the visitor walks
// c.sub(pos, len) or jumps over the record).
template <class C, class V>
PZ_CANON_FN bool walk_block(C& c, V&& v) {
  return walk_fields(c, 8, 0x4, 8, [&](uint32_t f, uint64_t q, uint64_t x) {
    if (f == 2) return v.scalar(f, x);
    if (f <= 6) return x && v.bytes(f, q, x);
    if (f == 8) return v.record(c, q, x);
    C t = c.sub(q, x);
    return walk_timestamp(t, v);
  });
}

// The bytes [p, e) of an input at `base`: positions are offsets from base.
struct PtrCursor {
  const uint8_t *base, *p, *e;
  bool ok;
  PZ_CANON_FN bool more() const { return p < e; }
  PZ_CANON_FN uint32_t next() { return *p++; }
  PZ_CANON_FN uint64_t left() const { return (uint64_t)(e - p); }
  PZ_CANON_FN uint64_t pos() const { return (uint64_t)(p - base); }
  PZ_CANON_FN void advance(uint64_t len) { p += len; }
  PZ_CANON_FN PtrCursor sub(uint64_t q, uint64_t len) const { return PtrCursor{base, base + q, base + q + len, true}; }
  // Jumps over a field of any wire type.  Not part of the rule: chain.hip's count_range only
  // counts a block's records with it; the parse that follows judges the block.
  void skip(uint32_t wt) {
    uint64_t q;
    if (wt == 0) get_varint(*this);
    else if (wt == 2) get_span(*this, get_varint(*this), &q);
    else if (wt == 1 && e - p >= 8) p += 8;
    else if (wt == 5 && e - p >= 4) p += 4;
    else ok = false;
  }
};

// 16 bytes at any alignment.  In the device pass a global load, not a flat one.
#ifdef __HIP_DEVICE_COMPILE__
__attribute__((device)) inline __attribute__((always_inline)) void load16(uint64_t (&v)[2], const uint8_t* s) {
  typedef __attribute__((address_space(1))) uint8_t gbyte;
  __builtin_memcpy(v, reinterpret_cast<const gbyte*>((uintptr_t)s), 16);
}
#else
inline void load16(uint64_t (&v)[2], const uint8_t* s) { std::memcpy(v, s, 16); }
#endif

// The bytes d[p, e) by offsets (no pointer is formed past the record).  Bytes come from a
// 16-byte window held in registers, loaded (unaligned) at min(pos, re - 16) inside the record
// d[rb, re): a key with its length or value is one load, where a load per varint byte was a
// dependent round trip each.  A record under 16 bytes, and WIN false, read byte by byte.
template <bool WIN>
struct OffsetCursor {
  const uint8_t* d;
  uint64_t p, e;
  bool ok;
  uint64_t rb, re;  // the record: what may be read
  uint64_t w;       // the window holds d[w, w + 16) (w = re: nothing yet)
  uint64_t win[2];
  static PZ_CANON_FN OffsetCursor over(const uint8_t* d, uint64_t beg, uint64_t end) {
    return OffsetCursor{d, beg, end, true, beg, end, end, {0, 0}};
  }
  PZ_CANON_FN bool more() const { return p < e; }
  PZ_CANON_FN uint64_t left() const { return e - p; }
  PZ_CANON_FN uint64_t pos() const { return p; }
  PZ_CANON_FN void advance(uint64_t len) { p += len; }
  PZ_CANON_FN OffsetCursor sub(uint64_t q, uint64_t len) const {  // (it starts with this cursor's window)
    return OffsetCursor{d, q, q + len, true, rb, re, w, {win[0], win[1]}};
  }
  PZ_CANON_FN uint32_t next() {
    const uint64_t at = p++;  // rb <= at < re
    if (!WIN || re - rb < 16) return d[at];
    if (at - w >= 16) {  // (unsigned: a window after `at`, or none yet, is far away too)
      w = at < re - 16 ? at : re - 16;
      load16(win, d + w);
    }
    const uint32_t off = (uint32_t)(at - w);
    return (uint32_t)((off < 8 ? win[0] >> (8 * off) : win[1] >> (8 * (off - 8))) & 0xff);
  }
};

}  // namespace canon
}  // namespace pz
