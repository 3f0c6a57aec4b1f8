// jpeg_parse_check.cpp -- the host half of the JPEG decoder (csrc/nid_jpeg_host.hpp) over untrusted bytes, as a stand-alone program
// for the address and undefined-behaviour sanitizers.  Host code only: it needs no GPU and must not be run on one.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I direct_visual_lidar_calibration_amd/csrc
//       tools/jpeg_parse_check.cpp -o jpeg_parse_check        (one command line)
//   python tests/make_jpeg_golden.py --dump-streams DIR      (the streams of tests/golden/jpeg_cases.npz as files)
//   ./jpeg_parse_check DIR/dri3_422.jpg DIR/adobe_420.jpg DIR/huff16_gray.jpg ...
//
// Per file: the whole stream, every prefix of it, and `kMutations` seeded single-byte mutations (the corpus of
// tests/test_jpeg_host.py, drawn with its own generator), each parsed with and without the entropy decode.  Every input must either
// parse or be refused with a reason; the sanitizers abort on anything else.  Exit status 0 and a count per file when all held.
#include "nid_jpeg_host.hpp"

#include <cstdio>
#include <fstream>
#include <iterator>

namespace {

constexpr int kMutations = 20000;

struct Tally {
  long parsed = 0, refused = 0;
};

bool run(const std::vector<uint8_t>& bytes, size_t n, Tally& t) {
  // a copy of exactly n bytes on the heap: a read past the end is a read past the allocation
  std::vector<uint8_t> exact(bytes.begin(), bytes.begin() + long(n));
  for (int entropy = 0; entropy < 2; entropy++) {
    nidjpeg::Stream s;
    std::string reason;
    const bool ok = nidjpeg::parse(exact.data(), exact.size(), entropy != 0, s, reason);
    if (!ok && reason.empty()) {
      std::fprintf(stderr, "refused without a reason (%zu bytes)\n", n);
      return false;
    }
    if (ok && entropy && s.coef.size() != s.total_blocks * 64) {
      std::fprintf(stderr, "parsed without its coefficients (%zu bytes)\n", n);
      return false;
    }
    (ok ? t.parsed : t.refused)++;
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s stream.jpg ...\n", argv[0]);
    return 2;
  }
  for (int a = 1; a < argc; a++) {
    std::ifstream f(argv[a], std::ios::binary);
    std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (bytes.empty()) {
      std::fprintf(stderr, "%s: empty or unreadable\n", argv[a]);
      return 2;
    }
    Tally t;
    for (size_t n = 0; n <= bytes.size(); n++)
      if (!run(bytes, n, t)) return 1;
    uint64_t state = 0x9E3779B97F4A7C15ull ^ uint64_t(a);
    for (int m = 0; m < kMutations; m++) {
      state = state * 6364136223846793005ull + 1442695040888963407ull;
      const size_t at = size_t((state >> 33) % bytes.size());
      const uint8_t value = uint8_t(state >> 24), old = bytes[at];
      bytes[at] = value;
      const bool ok = run(bytes, bytes.size(), t);
      bytes[at] = old;
      if (!ok) return 1;
    }
    std::printf("%s: %zu bytes, %zu prefixes, %d mutations: %ld parsed, %ld refused\n", argv[a], bytes.size(), bytes.size() + 1, kMutations, t.parsed, t.refused);
  }
  return 0;
}
