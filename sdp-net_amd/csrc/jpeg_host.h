// Host half of the hybrid JPEG decoder: marker parsing and the serial Huffman decode, in plain
// C++17 (no HIP include: libsdpnet_hip.so compiles it through jpeg_host.hip, and a stand-alone
// program can compile it as well, e.g. under a sanitizer -- tools/jpeg_host_check.cpp).
//
// No global state, no allocation, no call outside <stdint.h> / <string.h>: every function works on
// the caller's buffers and a Parser / Huff on its own stack, so any number of threads may decode at
// once.  Every read is bounds-checked against `len`, every write against `coef_cap`; a block is
// zeroed only right before it is decoded, and a block consumes at least two bits, so the work is
// O(len) whatever sizes the header claims.
//
// The contract (codes, info words, coefficient layout) is documented in include/sdpnet_hip.h.
#ifndef SDP_JPEG_HOST_H
#define SDP_JPEG_HOST_H
#include <stdint.h>
#include <string.h>

namespace sdpjpeg {

enum : int {
  OK = 0,
  // well-formed, not taken (the caller falls back to another decoder)
  UNS_PROGRESSIVE = 1,
  UNS_ARITHMETIC = 2,
  UNS_PRECISION = 3,   // 12-bit samples or 16-bit quantisation tables
  UNS_COMPONENTS = 4,  // neither 1 nor 3 components
  UNS_SAMPLING = 5,    // not luma 1x1 / 2x1 / 2x2 over chroma 1x1
  UNS_MULTISCAN = 6,
  UNS_DNL = 7,
  UNS_COLOUR = 8,      // three components that are not YCbCr (Adobe transform 0, ids "RGB")
  UNS_PROCESS = 9,     // lossless / hierarchical frames
  UNS_TOO_LARGE = 10,  // more than 2^31 - 1 coefficients
  // malformed
  ERR_TRUNCATED = -1,
  ERR_SYNTAX = -2,     // no SOI, a bad segment, a marker where none may stand
  ERR_CODE = -3,       // a bit pattern that is no code of the table
  ERR_INDEX = -4,      // a run that passes coefficient 63
  ERR_CATEGORY = -5,   // DC category above 11, AC category above 10, DC outside int16
  ERR_TABLE = -6,      // a table that was never defined
  ERR_RESTART = -7,    // a wrong or missing restart marker
  ERR_NO_EOI = -8,
  ERR_CAPACITY = -9,   // coef_cap below the coefficient count
  ERR_ARGUMENT = -10,
};

constexpr int INFO_WORDS = 16;
enum : int { I_W = 0, I_H, I_NCOMP, I_MODE, I_BW0, I_BH0, I_BW1, I_BH1, I_BW2, I_BH2, I_NCOEF, I_RESTART, I_MCUX, I_MCUY };

static const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int LOOK_BITS = 11;

struct Huff {
  bool defined = false;
  uint8_t vals[256];
  uint16_t look[1 << LOOK_BITS];  // prefix -> (length << 8) | symbol, 0: a longer code
  int16_t fast[1 << LOOK_BITS];   // AC only: (value << 8) | (run << 4) | (code + value bits) when those fit the
                                  // prefix and the value a signed byte, else 0
  int32_t maxcode[18];  // largest code of each length, -1: none
  int32_t valoff[17];   // vals index of a code = code + valoff[length]

  // counts[16], then the symbols; returns the bytes consumed or a negative code.
  int build(const uint8_t* p, int64_t avail) {
    if (avail < 16) return ERR_SYNTAX;
    int total = 0;
    for (int i = 0; i < 16; ++i) total += p[i];
    if (total > 256 || avail < 16 + total) return ERR_SYNTAX;
    memcpy(vals, p + 16, (size_t)total);
    memset(look, 0, sizeof(look));
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
      const int n = p[l - 1];
      if (code + n > (1 << l)) return ERR_SYNTAX;  // more codes than the length holds
      valoff[l] = k - code;
      if (l <= LOOK_BITS)
        for (int i = 0; i < n; ++i) {
          const int first = (code + i) << (LOOK_BITS - l);
          for (int f = 0; f < (1 << (LOOK_BITS - l)); ++f) look[first + f] = (uint16_t)((l << 8) | vals[k + i]);
        }
      k += n;
      code += n;
      maxcode[l] = n ? code - 1 : -1;
      code <<= 1;
    }
    maxcode[17] = 0x7fffffff;
    for (int i = 0; i < (1 << LOOK_BITS); ++i) {
      fast[i] = 0;
      const int len = look[i] >> 8, run = (look[i] >> 4) & 15, mag = look[i] & 15;
      if (len == 0 || mag == 0 || mag > 10 || len + mag > LOOK_BITS) continue;
      int v = ((i << len) & ((1 << LOOK_BITS) - 1)) >> (LOOK_BITS - mag);
      if (v < (1 << (mag - 1))) v += 1 - (1 << mag);
      if (v >= -128 && v <= 127) fast[i] = (int16_t)(v * 256 + run * 16 + len + mag);
    }
    defined = true;
    return 16 + total;
  }
};

// The marker code at pos with its fill bytes skipped (pos then stands behind it), or a negative code.
static inline int next_marker(const uint8_t* d, int64_t len, int64_t& pos) {
  if (pos >= len) return ERR_TRUNCATED;
  if (d[pos] != 0xFF) return ERR_SYNTAX;
  while (pos < len && d[pos] == 0xFF) ++pos;
  if (pos >= len) return ERR_TRUNCATED;
  return d[pos++];
}

struct Component {
  int id, h, v, tq, td, ta;
};

struct Parser {
  const uint8_t* d;
  int64_t len, pos;
  int W = 0, H = 0, ncomp = 0, mode = 0, hs = 1, vs = 1, mcux = 0, mcuy = 0, restart = 0;
  int adobe = -1;
  bool have_frame = false;
  Component comp[3];
  uint8_t qt[4][64];  // natural order
  bool qt_defined[4] = {false, false, false, false};
  Huff dc[4], ac[4];
  bool want_huff;

  Parser(const uint8_t* data, int64_t n, bool huff) : d(data), len(n), pos(0), want_huff(huff) {}

  int marker() { return next_marker(d, len, pos); }

  // Reads SOI .. SOS; 0 with pos at the first entropy-coded byte.
  int headers() {
    if (len < 2) return len >= 1 && d[0] != 0xFF ? ERR_SYNTAX : ERR_TRUNCATED;
    if (d[0] != 0xFF || d[1] != 0xD8) return ERR_SYNTAX;
    pos = 2;
    for (;;) {
      const int m = marker();
      if (m < 0) return m;
      if (m == 0xD8 || m == 0xD9 || m == 0x01 || m == 0x00 || (m >= 0xD0 && m <= 0xD7)) return ERR_SYNTAX;
      if (pos + 2 > len) return ERR_TRUNCATED;
      const int64_t n = ((int64_t)d[pos] << 8) | d[pos + 1];
      if (n < 2) return ERR_SYNTAX;
      if (pos + n > len) return ERR_TRUNCATED;
      const uint8_t* s = d + pos + 2;
      const int64_t sl = n - 2;
      pos += n;
      int rc = 0;
      if (m == 0xC0 || m == 0xC1) rc = frame(s, sl);
      else if (m == 0xC2) rc = UNS_PROGRESSIVE;
      else if (m == 0xC3 || (m >= 0xC5 && m <= 0xC7)) rc = UNS_PROCESS;
      else if (m == 0xCC || (m >= 0xC9 && m <= 0xCF)) rc = UNS_ARITHMETIC;
      else if (m == 0xC8) rc = ERR_SYNTAX;
      else if (m == 0xC4) rc = dht(s, sl);
      else if (m == 0xDB) rc = dqt(s, sl);
      else if (m == 0xDC) rc = UNS_DNL;
      else if (m == 0xDD) {
        if (sl != 2) return ERR_SYNTAX;
        restart = (s[0] << 8) | s[1];
      } else if (m == 0xEE) {
        if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) adobe = s[11];
      } else if (m == 0xDA) return scan(s, sl);
      if (rc) return rc;
    }
  }

  int frame(const uint8_t* s, int64_t sl) {
    if (have_frame) return ERR_SYNTAX;
    if (sl < 6) return ERR_SYNTAX;
    if (s[0] != 8) return s[0] == 12 || s[0] == 16 ? UNS_PRECISION : ERR_SYNTAX;
    H = (s[1] << 8) | s[2];
    W = (s[3] << 8) | s[4];
    const int nc = s[5];
    if (sl != 6 + 3 * (int64_t)nc || nc == 0) return ERR_SYNTAX;
    if (W == 0) return ERR_SYNTAX;
    if (H == 0) return UNS_DNL;
    if (nc != 1 && nc != 3) return UNS_COMPONENTS;
    ncomp = nc;
    for (int i = 0; i < nc; ++i) {
      Component& c = comp[i];
      c.id = s[6 + 3 * i];
      c.h = s[7 + 3 * i] >> 4;
      c.v = s[7 + 3 * i] & 15;
      c.tq = s[8 + 3 * i];
      c.td = c.ta = 0;
      if (c.h < 1 || c.h > 4 || c.v < 1 || c.v > 4 || c.tq > 3) return ERR_SYNTAX;
      for (int j = 0; j < i; ++j)
        if (comp[j].id == c.id) return ERR_SYNTAX;
    }
    have_frame = true;
    return 0;
  }

  int dht(const uint8_t* s, int64_t sl) {
    while (sl > 0) {
      const int tc = s[0] >> 4, th = s[0] & 15;
      if (tc > 1 || th > 3) return ERR_SYNTAX;
      Huff scratch;
      Huff& h = want_huff ? (tc ? ac[th] : dc[th]) : scratch;
      const int used = h.build(s + 1, sl - 1);
      if (used < 0) return used;
      if (!want_huff) (tc ? ac[th] : dc[th]).defined = true;
      s += 1 + used;
      sl -= 1 + used;
    }
    return 0;
  }

  int dqt(const uint8_t* s, int64_t sl) {
    while (sl > 0) {
      const int pq = s[0] >> 4, tq = s[0] & 15;
      if (pq > 1 || tq > 3) return ERR_SYNTAX;
      if (pq == 1) return sl < 129 ? ERR_SYNTAX : UNS_PRECISION;
      if (sl < 65) return ERR_SYNTAX;
      for (int k = 0; k < 64; ++k) qt[tq][kNatural[k]] = s[1 + k];
      qt_defined[tq] = true;
      s += 65;
      sl -= 65;
    }
    return 0;
  }

  int scan(const uint8_t* s, int64_t sl) {
    if (!have_frame) return ERR_SYNTAX;
    if (sl < 1) return ERR_SYNTAX;
    const int ns = s[0];
    if (ns < 1 || ns > 4 || sl != 4 + 2 * (int64_t)ns) return ERR_SYNTAX;
    if (ns != ncomp) return UNS_MULTISCAN;
    for (int i = 0; i < ns; ++i) {
      if (s[1 + 2 * i] != comp[i].id) return ERR_SYNTAX;
      comp[i].td = s[2 + 2 * i] >> 4;
      comp[i].ta = s[2 + 2 * i] & 15;
      if (comp[i].td > 3 || comp[i].ta > 3) return ERR_SYNTAX;
    }
    const uint8_t* t = s + 1 + 2 * ns;
    if (t[0] != 0 || t[1] != 63 || t[2] != 0) return ERR_SYNTAX;  // Ss, Se, Ah | Al of a sequential scan
    if (ncomp == 3) {
      if (adobe == 0 || (comp[0].id == 'R' && comp[1].id == 'G' && comp[2].id == 'B')) return UNS_COLOUR;
      if (comp[1].h != 1 || comp[1].v != 1 || comp[2].h != 1 || comp[2].v != 1) return UNS_SAMPLING;
      hs = comp[0].h;
      vs = comp[0].v;
      if (hs == 1 && vs == 1) mode = 0;
      else if (hs == 2 && vs == 1) mode = 1;
      else if (hs == 2 && vs == 2) mode = 2;
      else return UNS_SAMPLING;
    } else {
      hs = vs = 1;  // a single-component scan is not interleaved: one block per MCU
      mode = 0;
    }
    mcux = (W + 8 * hs - 1) / (8 * hs);
    mcuy = (H + 8 * vs - 1) / (8 * vs);
    if (ncoef() > 0x7fffffff) return UNS_TOO_LARGE;
    for (int i = 0; i < ncomp; ++i)
      if (!qt_defined[comp[i].tq] || !dc[comp[i].td].defined || !ac[comp[i].ta].defined) return ERR_TABLE;
    return 0;
  }

  int64_t ncoef() const {
    return 64 * ((int64_t)mcux * hs * mcuy * vs + (ncomp == 3 ? 2 * (int64_t)mcux * mcuy : 0));
  }

  void fill_info(int32_t* info) const {
    for (int i = 0; i < INFO_WORDS; ++i) info[i] = 0;
    info[I_W] = W;
    info[I_H] = H;
    info[I_NCOMP] = ncomp;
    info[I_MODE] = mode;
    info[I_BW0] = mcux * hs;
    info[I_BH0] = mcuy * vs;
    if (ncomp == 3) {
      info[I_BW1] = info[I_BW2] = mcux;
      info[I_BH1] = info[I_BH2] = mcuy;
    }
    info[I_NCOEF] = (int32_t)ncoef();
    info[I_RESTART] = restart;
    info[I_MCUX] = mcux;
    info[I_MCUY] = mcuy;
  }
};

// Bit reader over the entropy-coded segment: the accumulator is left-aligned, FF00 yields FF, and
// any other FF xx stops the refill (pos stays on the FF), so a marker is never read as data.
struct Bits {
  const uint8_t* d;
  int64_t len, pos;
  uint64_t acc = 0;
  int n = 0;

  void fill() {
    if (n <= 32 && pos + 4 <= len) {  // four bytes at once when none of them is FF
      const uint32_t w = ((uint32_t)d[pos] << 24) | ((uint32_t)d[pos + 1] << 16) | ((uint32_t)d[pos + 2] << 8) | d[pos + 3];
      const uint32_t v = ~w;
      if (((v - 0x01010101u) & ~v & 0x80808080u) == 0) {
        acc |= (uint64_t)w << (32 - n);
        n += 32;
        pos += 4;
        return;
      }
    }
    while (n <= 56 && pos < len) {
      const uint8_t b = d[pos];
      if (b == 0xFF) {
        if (pos + 1 >= len || d[pos + 1] != 0) break;
        pos += 2;
      } else {
        ++pos;
      }
      acc |= (uint64_t)b << (56 - n);
      n += 8;
    }
  }
  uint32_t peek(int k) const { return (uint32_t)(acc >> (64 - k)); }
  void drop(int k) {
    acc <<= k;
    n -= k;
  }
  // One Huffman symbol; the caller has refilled (27 bits cover a code and its value bits).
  // ERR_TRUNCATED when the data ends or a marker cuts it short, ERR_CODE for an unknown code.
  int symbol(const Huff& h) {
    const uint16_t e = h.look[peek(LOOK_BITS)];
    int l, sym;
    if (e) {
      l = e >> 8;
      sym = e & 255;
    } else {
      l = LOOK_BITS + 1;
      while ((int32_t)peek(l) > h.maxcode[l]) ++l;
      if (l > 16) return ERR_CODE;
      sym = h.vals[(int32_t)peek(l) + h.valoff[l]];
    }
    if (l > n) return ERR_TRUNCATED;
    drop(l);
    return sym;
  }
  // s in 1..16 bits, sign-extended as JPEG's EXTEND; ok = false when the bits are not there.
  int receive(int s, bool& ok) {
    if (n < s) {
      ok = false;
      return 0;
    }
    const int v = (int)peek(s);
    drop(s);
    return v + (((v - (1 << (s - 1))) >> 31) & (1 - (1 << s)));
  }
};

static inline int decode_block(Bits& br, const Huff& dc, const Huff& ac, int& pred, int16_t* out) {
  memset(out, 0, 64 * sizeof(int16_t));
  bool ok = true;
  if (br.n < 32) br.fill();
  int s = br.symbol(dc);
  if (s < 0) return s;
  if (s > 11) return ERR_CATEGORY;
  if (s) pred += br.receive(s, ok);
  if (!ok) return ERR_TRUNCATED;
  if (pred < -32768 || pred > 32767) return ERR_CATEGORY;
  out[0] = (int16_t)pred;
  int k = 1;
  while (k < 64) {
    if (br.n < 32) br.fill();
    const int f = ac.fast[br.peek(LOOK_BITS)];
    if (f) {  // a short code and its value bits in one look-up
      const int used = f & 15;
      if (used > br.n) return ERR_TRUNCATED;
      k += (f >> 4) & 15;
      if (k > 63) return ERR_INDEX;
      br.drop(used);
      out[kNatural[k++]] = (int16_t)(f >> 8);
      continue;
    }
    const int rs = br.symbol(ac);
    if (rs < 0) return rs;
    const int r = rs >> 4;
    s = rs & 15;
    if (s) {
      if (s > 10) return ERR_CATEGORY;
      k += r;
      if (k > 63) return ERR_INDEX;
      out[kNatural[k]] = (int16_t)br.receive(s, ok);
      if (!ok) return ERR_TRUNCATED;
      ++k;
    } else if (r == 15) {
      k += 16;
      if (k > 64) return ERR_INDEX;
    } else if (r == 0) {
      break;
    } else {
      return ERR_CODE;  // EOBn belongs to progressive scans
    }
  }
  return 0;
}

inline int probe(const uint8_t* data, int64_t len, int32_t* info) {
  if (!data || !info || len < 0) return ERR_ARGUMENT;
  for (int i = 0; i < INFO_WORDS; ++i) info[i] = 0;
  Parser p(data, len, false);
  const int rc = p.headers();
  if (rc == 0) p.fill_info(info);
  return rc;
}

// qt: uint8 [3][64], natural order, table of component c at qt + 64 c (zero for absent components).
inline int entropy_decode(const uint8_t* data, int64_t len, int16_t* coef, int64_t coef_cap, uint8_t* qt,
                          int32_t* info) {
  if (!data || !info || !coef || !qt || len < 0 || coef_cap < 0) return ERR_ARGUMENT;
  for (int i = 0; i < INFO_WORDS; ++i) info[i] = 0;
  Parser p(data, len, true);
  int rc = p.headers();
  if (rc) return rc;
  p.fill_info(info);
  if (p.ncoef() > coef_cap) return ERR_CAPACITY;
  memset(qt, 0, 192);
  for (int c = 0; c < p.ncomp; ++c) memcpy(qt + 64 * c, p.qt[p.comp[c].tq], 64);

  Bits br{data, len, p.pos};
  const int bw0 = p.mcux * p.hs;
  int16_t* base[3] = {coef, coef + 64 * (int64_t)bw0 * p.mcuy * p.vs,
                      coef + 64 * ((int64_t)bw0 * p.mcuy * p.vs + (int64_t)p.mcux * p.mcuy)};
  int pred[3] = {0, 0, 0};
  int next_rst = 0, left = p.restart;
  for (int my = 0; my < p.mcuy; ++my)
    for (int mx = 0; mx < p.mcux; ++mx) {
      if (p.restart && left == 0) {
        // the padding of the last byte goes, whole unread bytes may not stand before the marker
        if (br.n >= 8) return ERR_RESTART;
        br.acc = 0;
        br.n = 0;
        const int mk = next_marker(data, len, br.pos);
        if (mk == ERR_TRUNCATED) return ERR_TRUNCATED;
        if (mk != 0xD0 + next_rst) return ERR_RESTART;
        next_rst = (next_rst + 1) & 7;
        pred[0] = pred[1] = pred[2] = 0;
        left = p.restart;
      }
      --left;
      for (int v = 0; v < p.vs; ++v)
        for (int h = 0; h < p.hs; ++h) {
          int16_t* out = base[0] + 64 * ((int64_t)(my * p.vs + v) * bw0 + mx * p.hs + h);
          rc = decode_block(br, p.dc[p.comp[0].td], p.ac[p.comp[0].ta], pred[0], out);
          if (rc) return rc;
        }
      for (int c = 1; c < p.ncomp; ++c) {
        int16_t* out = base[c] + 64 * ((int64_t)my * p.mcux + mx);
        rc = decode_block(br, p.dc[p.comp[c].td], p.ac[p.comp[c].ta], pred[c], out);
        if (rc) return rc;
      }
    }
  if (br.n >= 8) return ERR_SYNTAX;  // whole bytes of entropy data past the last MCU
  const int mk = next_marker(data, len, br.pos);
  if (mk == 0xD9) return 0;
  if (mk == ERR_TRUNCATED || mk == ERR_SYNTAX) return ERR_NO_EOI;
  if (mk == 0xDC) return UNS_DNL;
  if (mk >= 0xD0 && mk <= 0xD7) return ERR_RESTART;
  if (mk == 0xDA || mk == 0xC4 || mk == 0xDB || mk == 0xDD) return UNS_MULTISCAN;
  return ERR_SYNTAX;
}

}  // namespace sdpjpeg
#endif  // SDP_JPEG_HOST_H
