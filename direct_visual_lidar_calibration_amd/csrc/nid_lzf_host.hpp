// nid_lzf_host.hpp -- an LZF decoder for the body of a PCD file stored as `DATA binary_compressed` (dataset.read_pcd), written from
// the public description of the stream.  Plain C++, no HIP header: it compiles alone with g++ (tools/lzf_check.cpp runs it under
// the address and undefined-behaviour sanitizers).  UNPINNED against liblzf / PCL and real files: neither is available to the
// tests, which use hand-assembled streams (tests/las_oracle.py).
//
// The stream is a sequence of tokens.  A control byte c < 32 starts a literal run: the next c + 1 bytes are copied to the output.
// Any other control byte is a back-reference: length (c >> 5) + 2 -- when the 3-bit field is 7, one further byte is added to the
// length --, then one byte that is the low part of the distance: distance = ((c & 31) << 8 | low) + 1, at most 8192, counted back
// from the write position.  The copy runs byte by byte, so a reference that overlaps its own output replicates (distance 1 = a run).
// Every read and every write is bounds-checked; the input is untrusted.  Refused, each with the input offset of the token: input
// that ends inside a token, a reference to before the start of the output, and output past out_size.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace nidlzf {

// `written` = bytes of output produced (also on refusal: what was produced before it).  An empty input decodes to nothing.
inline bool decompress(const uint8_t* in, size_t in_size, uint8_t* out, size_t out_size, size_t& written, std::string& reason) {
  size_t ip = 0, op = 0;
  written = 0;
  const auto refuse = [&](size_t at, const char* what) {
    written = op;
    reason = std::string(what) + " (token at input offset " + std::to_string(at) + ", " + std::to_string(op) + " bytes written)";
    return false;
  };
  while (ip < in_size) {
    const size_t at = ip;
    const unsigned ctrl = in[ip++];
    if (ctrl < 32) {
      const size_t run = size_t(ctrl) + 1;
      if (run > in_size - ip) return refuse(at, "LZF input ends inside a literal run");
      if (run > out_size - op) return refuse(at, "LZF literal run overruns the output");
      for (size_t k = 0; k < run; k++) out[op++] = in[ip++];
    } else {
      size_t len = ctrl >> 5;
      if (len == 7) {
        if (ip >= in_size) return refuse(at, "LZF input ends inside a back-reference");
        len += in[ip++];
      }
      if (ip >= in_size) return refuse(at, "LZF input ends inside a back-reference");
      const size_t dist = ((size_t(ctrl & 31) << 8) | in[ip++]) + 1;
      len += 2;
      if (dist > op) return refuse(at, "LZF back-reference starts before the output");
      if (len > out_size - op) return refuse(at, "LZF back-reference overruns the output");
      for (size_t k = 0; k < len; k++, op++) out[op] = out[op - dist];  // byte by byte: an overlapping copy replicates
    }
  }
  written = op;
  return true;
}

}  // namespace nidlzf
