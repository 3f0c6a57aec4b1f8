// nid_jpeg_host.hpp -- the host half of the baseline JPEG decoder (include/nidreg.h: nidreg_jpeg_*): marker parser, Huffman table
// build and entropy decode to quantised int16 blocks.  No HIP header: this file compiles alone with g++ (tools/jpeg_parse_check.cpp
// runs it under the address and undefined-behaviour sanitizers).  Everything arithmetic on the samples -- dequantisation, inverse
// DCT, upsampling, colour -- is device code (nid_jpeg_kernels.hpp).
//
// The bytes are untrusted: every read is bounds-checked against `size`, nothing is allocated from a declared size before the entropy
// data is known to be long enough to fill it (two bits per block at the least), and every refusal is a reason string, never an abort.
// What is accepted and what is refused is listed in include/nidreg.h.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace nidjpeg {

enum Subsampling { kGray = 0, k444 = 1, k422 = 2, k420 = 3 };

// zig-zag position -> natural (row-major) position
static const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffTable {
  bool set = false;
  uint8_t bits[17] = {0};     // bits[l]: number of codes of length l
  uint8_t vals[256] = {0};
  int32_t maxcode[18] = {0};  // largest code of length l, -1 when there is none; [17] is a sentinel that ends every walk
  int32_t valptr[17] = {0};   // index into vals of the first code of length l, minus that code
  int16_t look[256] = {0};    // the next 8 bits -> (length << 8) | symbol, 0 when the code is longer than 8 bits
};

struct Component {
  int id = 0, h = 1, v = 1, tq = 0, td = 0, ta = 0;
  int bw = 0, bh = 0;     // the component's full block grid (whole MCUs)
  int dw = 0, dh = 0;     // its downsampled size: ceil(W h / hmax) x ceil(H v / vmax), where the edges are
  size_t block_offset = 0;  // first block in Stream::coef
};

struct Stream {
  int width = 0, height = 0, ncomp = 0, subsampling = kGray, orientation = 1;
  int hmax = 1, vmax = 1, mcux = 0, mcuy = 0, restart_interval = 0;
  Component comp[3];
  uint16_t qt[4][64] = {{0}};  // natural order
  bool qt_set[4] = {false, false, false, false};
  HuffTable dc[4], ac[4];
  std::vector<int16_t> coef;  // per component, raster order over its full block grid, 64 natural-order coefficients a block
  size_t total_blocks = 0;
};

namespace detail {

inline bool build_huffman(HuffTable& t, bool is_dc, std::string& reason) {
  int total = 0;
  for (int l = 1; l <= 16; l++) total += t.bits[l];
  // (total <= 256 is checked by the caller against the segment)
  int32_t code = 0;
  int p = 0;
  std::memset(t.look, 0, sizeof(t.look));
  for (int l = 1; l <= 16; l++) {
    if (t.bits[l] == 0) {
      t.maxcode[l] = -1;
    } else {
      if (code + t.bits[l] >= (1 << l)) {  // (libjpeg's rule: the all-ones code of a length stays unused); checked BEFORE a code indexes the table
        reason = "a Huffman table whose code lengths do not form a prefix code";
        return false;
      }
      t.valptr[l] = p - code;
      for (int i = 0; i < t.bits[l]; i++, p++, code++) {
        if (l <= 8) {
          const int first = code << (8 - l);
          for (int k = 0; k < (1 << (8 - l)); k++) t.look[first + k] = int16_t((l << 8) | t.vals[p]);
        }
      }
      t.maxcode[l] = code - 1;
    }
    code <<= 1;
  }
  t.maxcode[17] = 0x7fffffff;
  if (is_dc)
    for (int i = 0; i < total; i++)
      if (t.vals[i] > 15) {
        reason = "a DC Huffman table with a category above 15";
        return false;
      }
  t.set = true;
  return true;
}

// The entropy-coded segment as a stream of bits: 0xFF00 is the byte 0xFF, a run of 0xFF before a marker is fill, and a marker (or
// the end of the data) ends the supply -- a request past it is the truncation that is refused.
struct BitReader {
  const uint8_t* data;
  size_t size, pos;
  uint64_t buf = 0;
  int cnt = 0;
  bool at_marker = false;  // pos is at the 0xFF of a marker, or at the end of the data

  BitReader(const uint8_t* d, size_t n, size_t p) : data(d), size(n), pos(p) {}

  void fill() {
    while (cnt <= 56 && !at_marker) {
      if (pos >= size) {
        at_marker = true;
        break;
      }
      const uint8_t c = data[pos];
      if (c == 0xFF) {
        size_t q = pos + 1;
        while (q < size && data[q] == 0xFF) q++;
        if (q >= size) {
          pos = size;
          at_marker = true;
          break;
        }
        if (data[q] != 0) {
          pos = q - 1;
          at_marker = true;
          break;
        }
        pos = q + 1;
      } else {
        pos++;
      }
      buf = (buf << 8) | c;
      cnt += 8;
    }
  }
  // n in [1, 16]; false when the data ended first
  bool get(int n, int& out) {
    if (cnt < n) {
      fill();
      if (cnt < n) return false;
    }
    out = int((buf >> (cnt - n)) & ((1u << n) - 1u));
    cnt -= n;
    return true;
  }
  // 0: a symbol; 1: data ended; 2: no such code
  int decode(const HuffTable& t, int& sym) {
    if (cnt < 16) fill();
    if (cnt >= 8) {
      const int e = t.look[(buf >> (cnt - 8)) & 0xFF];
      if (e) {
        cnt -= e >> 8;
        sym = e & 0xFF;
        return 0;
      }
    }
    int32_t code = 0;
    for (int l = 1; l <= 16; l++) {
      int b;
      if (!get(1, b)) return 1;
      code = (code << 1) | b;
      if (code <= t.maxcode[l]) {
        sym = t.vals[t.valptr[l] + code];
        return 0;
      }
    }
    return 2;
  }
  // between two restart intervals: drop the padding bits, then the marker that must follow; its code, or -1 at the end of the data
  int restart_marker() {
    buf = 0, cnt = 0;
    if (!at_marker) {  // bytes that no MCU used: skipped, as libjpeg's next_marker skips them
      while (pos + 1 < size && !(data[pos] == 0xFF && data[pos + 1] != 0 && data[pos + 1] != 0xFF)) pos++;
      if (pos + 1 >= size) pos = size;
    }
    if (pos + 1 >= size) return -1;
    const int m = data[pos + 1];
    pos += 2;
    at_marker = false;
    return m;
  }
};

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

inline int exif_orientation(const uint8_t* p, size_t n) {
  // p: the APP1 payload after the length.  "Exif\0\0", then a TIFF header: byte order, 42, the offset of IFD0
  if (n < 14 || std::memcmp(p, "Exif\0\0", 6) != 0) return 0;
  const uint8_t* t = p + 6;
  const size_t tn = n - 6;
  bool le;
  if (t[0] == 'I' && t[1] == 'I')
    le = true;
  else if (t[0] == 'M' && t[1] == 'M')
    le = false;
  else
    return 0;
  auto u16 = [&](size_t o) -> uint32_t { return le ? uint32_t(t[o] | (t[o + 1] << 8)) : uint32_t((t[o] << 8) | t[o + 1]); };
  auto u32 = [&](size_t o) -> uint32_t { return le ? (u16(o) | (u16(o + 2) << 16)) : ((u16(o) << 16) | u16(o + 2)); };
  if (u16(2) != 42) return 0;
  const size_t ifd = u32(4);
  if (ifd > tn || tn - ifd < 2) return 0;
  const size_t count = u16(ifd);
  for (size_t i = 0; i < count; i++) {
    const size_t e = ifd + 2 + 12 * i;
    if (e > tn || tn - e < 12) return 0;
    if (u16(e) == 0x0112) {
      if (u16(e + 2) != 3 || u32(e + 4) != 1) return 0;  // one SHORT
      const uint32_t v = u16(e + 8);
      return v >= 1 && v <= 8 ? int(v) : 0;
    }
  }
  return 0;
}

}  // namespace detail

// Parses the stream up to its one scan and, when `entropy` is set, decodes that scan into s.coef.  Returns false with `reason`
// filled in for everything that is refused.
inline bool parse(const uint8_t* data, size_t size, bool entropy, Stream& s, std::string& reason) {
  using namespace detail;
  if (!data || size < 4 || data[0] != 0xFF || data[1] != 0xD8) {
    reason = "no SOI marker at the start";
    return false;
  }
  size_t pos = 2;
  bool have_sof = false, saw_jfif = false, saw_adobe = false, have_exif = false;
  int adobe_transform = 0;
  for (;;) {
    // a marker: 0xFF, any number of 0xFF fill bytes, the code
    if (pos >= size || data[pos] != 0xFF) {
      reason = pos >= size ? "the data ends before the scan" : "a byte that is no marker between two segments";
      return false;
    }
    while (pos < size && data[pos] == 0xFF) pos++;
    if (pos >= size) {
      reason = "the data ends before the scan";
      return false;
    }
    const int m = data[pos++];
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // TEM, a stray RSTn: no payload
    if (m == 0x00) {
      reason = "a byte that is no marker between two segments";
      return false;
    }
    if (m == 0xD8) {
      reason = "a second SOI marker";
      return false;
    }
    if (m == 0xD9) {
      reason = "EOI before any scan";
      return false;
    }
    if (size - pos < 2) {
      reason = "the data ends inside a segment";
      return false;
    }
    const size_t len = (size_t(data[pos]) << 8) | data[pos + 1];
    if (len < 2 || len > size - pos) {
      reason = "a segment length that is below 2 or runs past the data";
      return false;
    }
    const uint8_t* p = data + pos + 2;
    const size_t n = len - 2;
    pos += len;
    if (m == 0xC2 || m == 0xC6 || m == 0xCA || m == 0xCE) {
      reason = m == 0xC2 ? "a progressive stream (SOF2)" : "a progressive, differential or arithmetic-coded stream";
      return false;
    }
    if (m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF) {
      reason = "a lossless stream";
      return false;
    }
    if (m == 0xC9 || m == 0xCD || m == 0xCC) {
      reason = "an arithmetic-coded stream";
      return false;
    }
    if (m == 0xC5) {
      reason = "a differential (hierarchical) stream";
      return false;
    }
    if (m == 0xC0 || m == 0xC1) {
      if (have_sof) {
        reason = "a second frame header";
        return false;
      }
      if (n < 6) {
        reason = "a frame header that is too short";
        return false;
      }
      if (p[0] != 8) {
        reason = "sample precision " + std::to_string(int(p[0])) + " (a 12-bit stream), only 8 is decoded";
        return false;
      }
      s.height = (p[1] << 8) | p[2];
      s.width = (p[3] << 8) | p[4];
      s.ncomp = p[5];
      if (s.width == 0 || s.height == 0 || s.width > 32768 || s.height > 32768) {
        reason = "dimensions " + std::to_string(s.width) + " x " + std::to_string(s.height) + " outside [1, 32768]";
        return false;
      }
      if (s.ncomp != 1 && s.ncomp != 3) {
        reason = std::to_string(s.ncomp) + " components (1, or 3 coded as YCbCr, are decoded)";
        return false;
      }
      if (n != size_t(6 + 3 * s.ncomp)) {
        reason = "a frame header whose length does not match its component count";
        return false;
      }
      for (int c = 0; c < s.ncomp; c++) {
        Component& k = s.comp[c];
        k.id = p[6 + 3 * c];
        k.h = p[7 + 3 * c] >> 4;
        k.v = p[7 + 3 * c] & 15;
        k.tq = p[8 + 3 * c];
        if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4 || k.tq > 3) {
          reason = "a sampling factor outside [1, 4] or a quantisation table index above 3";
          return false;
        }
        for (int d = 0; d < c; d++)
          if (s.comp[d].id == k.id) {
            reason = "two components with the same identifier";
            return false;
          }
      }
      have_sof = true;
      continue;
    }
    if (m == 0xC4) {  // DHT: any number of tables
      size_t o = 0;
      while (o < n) {
        if (n - o < 17) {
          reason = "a Huffman table segment that is too short";
          return false;
        }
        const int tc = p[o] >> 4, th = p[o] & 15;
        if (tc > 1 || th > 3) {
          reason = "a Huffman table class above 1 or index above 3";
          return false;
        }
        HuffTable& t = tc ? s.ac[th] : s.dc[th];
        t = HuffTable();
        int total = 0;
        for (int l = 1; l <= 16; l++) total += (t.bits[l] = p[o + l]);
        o += 17;
        if (total > 256 || size_t(total) > n - o) {
          reason = "a Huffman table with more symbols than its segment holds";
          return false;
        }
        std::memcpy(t.vals, p + o, size_t(total));
        o += size_t(total);
        if (!build_huffman(t, tc == 0, reason)) return false;
      }
      continue;
    }
    if (m == 0xDB) {  // DQT: any number of tables, 8- or 16-bit entries, zig-zag order
      size_t o = 0;
      while (o < n) {
        const int pq = p[o] >> 4, tq = p[o] & 15;
        if (pq > 1 || tq > 3) {
          reason = "a quantisation table precision above 1 or index above 3";
          return false;
        }
        const size_t need = pq ? 128 : 64;
        if (n - o - 1 < need) {
          reason = "a quantisation table segment that is too short";
          return false;
        }
        for (int i = 0; i < 64; i++) s.qt[tq][kNatural[i]] = pq ? uint16_t((p[o + 1 + 2 * i] << 8) | p[o + 2 + 2 * i]) : uint16_t(p[o + 1 + i]);
        s.qt_set[tq] = true;
        o += 1 + need;
      }
      continue;
    }
    if (m == 0xDD) {
      if (n != 2) {
        reason = "a restart interval segment of the wrong length";
        return false;
      }
      s.restart_interval = (p[0] << 8) | p[1];
      continue;
    }
    if (m == 0xE0) {
      if (n >= 14 && std::memcmp(p, "JFIF\0", 5) == 0) saw_jfif = true;
      continue;
    }
    if (m == 0xE1) {
      if (!have_exif) {
        const int o = exif_orientation(p, n);
        if (o) s.orientation = o, have_exif = true;
      }
      continue;
    }
    if (m == 0xEE) {
      if (n >= 12 && std::memcmp(p, "Adobe", 5) == 0) saw_adobe = true, adobe_transform = p[11];
      continue;
    }
    if (m != 0xDA) continue;  // APPn, COM, DNL, ...: skipped

    // ---- SOS: the one scan
    if (!have_sof) {
      reason = "a scan before the frame header";
      return false;
    }
    if (n >= 1 && int(p[0]) != s.ncomp && p[0] >= 1 && p[0] <= 4) {
      reason = "a non-interleaved (multi-scan) file: the scan holds " + std::to_string(int(p[0])) + " of " + std::to_string(s.ncomp) + " components";
      return false;
    }
    if (n < 1 || int(p[0]) != s.ncomp || n != size_t(4 + 2 * s.ncomp)) {
      reason = "a scan header of the wrong length";
      return false;
    }
    for (int c = 0; c < s.ncomp; c++) {
      Component& k = s.comp[c];
      if (int(p[1 + 2 * c]) != k.id) {
        reason = "a scan whose components are not the frame's, in the frame's order";
        return false;
      }
      k.td = p[2 + 2 * c] >> 4;
      k.ta = p[2 + 2 * c] & 15;
      if (k.td > 3 || k.ta > 3 || !s.dc[k.td].set || !s.ac[k.ta].set) {
        reason = "a missing Huffman table (component " + std::to_string(c) + ")";
        return false;
      }
      if (!s.qt_set[k.tq]) {
        reason = "a missing quantisation table (component " + std::to_string(c) + ")";
        return false;
      }
    }
    break;
  }

  // ---- colour space (libjpeg's rule) and sampling
  if (s.ncomp == 3) {
    if (saw_jfif) {
    } else if (saw_adobe) {
      if (adobe_transform == 0 || adobe_transform == 2) {
        reason = adobe_transform == 0 ? "Adobe transform 0: the components are RGB, not YCbCr" : "Adobe transform 2 (YCCK)";
        return false;
      }
    } else if (s.comp[0].id == 'R' && s.comp[1].id == 'G' && s.comp[2].id == 'B') {
      reason = "component identifiers R, G, B without a JFIF or Adobe marker: the components are RGB, not YCbCr";
      return false;
    }
    const Component &y = s.comp[0], &cb = s.comp[1], &cr = s.comp[2];
    if (cb.h != 1 || cb.v != 1 || cr.h != 1 || cr.v != 1 || !((y.h == 1 && y.v == 1) || (y.h == 2 && y.v == 1) || (y.h == 2 && y.v == 2))) {
      reason = "sampling factors " + std::to_string(y.h) + "x" + std::to_string(y.v) + ", " + std::to_string(cb.h) + "x" + std::to_string(cb.v) + ", " + std::to_string(cr.h) + "x" +
               std::to_string(cr.v) + " (4:4:4, 4:2:2 and 4:2:0 with 1x1 chroma are decoded)";
      return false;
    }
    s.subsampling = y.h == 1 ? k444 : (y.v == 1 ? k422 : k420);
    s.hmax = y.h, s.vmax = y.v;
  } else {
    s.comp[0].h = s.comp[0].v = 1;  // one component: the scan is not interleaved, its factors mean nothing (as in libjpeg)
    s.subsampling = kGray;
    s.hmax = s.vmax = 1;
  }
  s.mcux = (s.width + 8 * s.hmax - 1) / (8 * s.hmax);
  s.mcuy = (s.height + 8 * s.vmax - 1) / (8 * s.vmax);
  size_t blocks = 0;
  int per_mcu = 0;
  for (int c = 0; c < s.ncomp; c++) {
    Component& k = s.comp[c];
    k.bw = s.mcux * k.h, k.bh = s.mcuy * k.v;
    k.dw = (s.width * k.h + s.hmax - 1) / s.hmax, k.dh = (s.height * k.v + s.vmax - 1) / s.vmax;
    k.block_offset = blocks;
    blocks += size_t(k.bw) * size_t(k.bh);
    per_mcu += k.h * k.v;
  }
  s.total_blocks = blocks;
  if (!entropy) return true;

  // ---- entropy decode.  A block costs two bits at the least (a DC code and an EOB): refuse before allocating what cannot be filled.
  const size_t mcus = size_t(s.mcux) * size_t(s.mcuy);
  if ((size - pos) * 8 < mcus * size_t(per_mcu) * 2) {
    reason = "entropy data that ends before the last MCU";
    return false;
  }
  s.coef.assign(blocks * 64, 0);
  BitReader br(data, size, pos);
  int pred[3] = {0, 0, 0};
  int until_restart = s.restart_interval, next_rst = 0;
  size_t mcu = 0;
  for (int my = 0; my < s.mcuy; my++) {
    for (int mx = 0; mx < s.mcux; mx++, mcu++) {
      if (s.restart_interval && until_restart == 0) {
        const int m = br.restart_marker();
        if (m != 0xD0 + next_rst) {
          reason = m < 0 ? "entropy data that ends before the last MCU" : "a restart marker that is missing or out of sequence";
          return false;
        }
        next_rst = (next_rst + 1) & 7;
        until_restart = s.restart_interval;
        pred[0] = pred[1] = pred[2] = 0;
      }
      until_restart--;
      for (int c = 0; c < s.ncomp; c++) {
        const Component& k = s.comp[c];
        const HuffTable &dct = s.dc[k.td], &act = s.ac[k.ta];
        for (int by = 0; by < k.v; by++) {
          for (int bx = 0; bx < k.h; bx++) {
            int16_t* blk = s.coef.data() + (k.block_offset + size_t(my * k.v + by) * size_t(k.bw) + size_t(mx * k.h + bx)) * 64;
            int sym = 0, bits = 0;
            int st = br.decode(dct, sym);
            if (st == 0 && sym) {
              if (!br.get(sym, bits)) st = 1;
              else pred[c] = int16_t(pred[c] + extend(bits, sym));
            }
            if (st) {
              reason = st == 1 ? "entropy data that ends before the last MCU" : "a Huffman code that does not exist";
              return false;
            }
            blk[0] = int16_t(pred[c]);
            for (int kk = 1; kk < 64; kk++) {
              st = br.decode(act, sym);
              if (st) {
                reason = st == 1 ? "entropy data that ends before the last MCU" : "a Huffman code that does not exist";
                return false;
              }
              const int r = sym >> 4, sz = sym & 15;
              if (sz == 0) {
                if (r != 15) break;  // EOB
                kk += 15;            // ZRL (one that runs past 63 ends the block, as in libjpeg)
                continue;
              }
              kk += r;
              if (kk > 63) {
                reason = "a zero run past coefficient 63";
                return false;
              }
              if (!br.get(sz, bits)) {
                reason = "entropy data that ends before the last MCU";
                return false;
              }
              blk[kNatural[kk]] = int16_t(extend(bits, sz));
            }
          }
        }
      }
    }
  }
  return true;
}

}  // namespace nidjpeg
