// Host run of electionguard-remote_amd/csrc/eg_u256.hpp (tests/test_u256.py compiles and runs it):
// the same bodies the device kernels inline, as plain host code.  The wrapper draws the operands
// and knows the answers; this program only reads "op operand ..." lines (operands in hex, 256-bit
// ones as 64 digits), runs the function and prints what it got, one line per case.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "eg_u256.hpp"

using eg::U256;

// 32 big-endian bytes in word-aligned storage: ld256 and st256 move whole words
struct Be32 {
  alignas(16) uint32_t words[8];
  uint8_t* bytes() { return reinterpret_cast<uint8_t*>(words); }
};

static int nibble(char c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  if (c >= 'A' && c <= 'F') return c - 'A' + 10;
  std::fprintf(stderr, "bad hex digit '%c'\n", c);
  std::exit(2);
}

static U256 scalar(const std::string& hex) {
  if (hex.size() != 64) {
    std::fprintf(stderr, "a scalar is 64 hex digits, got %zu\n", hex.size());
    std::exit(2);
  }
  Be32 b;
  for (int i = 0; i < 32; ++i) b.bytes()[i] = (uint8_t)(nibble(hex[2 * i]) << 4 | nibble(hex[2 * i + 1]));
  return eg::ld256(b.bytes());
}

static uint32_t word(const std::string& hex) { return (uint32_t)std::strtoul(hex.c_str(), nullptr, 16); }

static void print(const U256& a) {
  Be32 b;
  eg::st256(b.bytes(), a);
  for (int i = 0; i < 32; ++i) std::printf("%02x", b.bytes()[i]);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char line[512];
  while (std::fgets(line, sizeof line, f)) {
    std::vector<std::string> t;
    for (char* p = std::strtok(line, " \n"); p; p = std::strtok(nullptr, " \n")) t.push_back(p);
    if (t.empty()) continue;
    const std::string& op = t[0];
    auto S = [&](size_t i) { return scalar(t.at(i)); };
    if (op == "words") {  // ld256's word order: w[0] is the least significant
      const U256 a = S(1);
      for (int i = 7; i >= 0; --i) std::printf("%08x", a.w[i]);
    } else if (op == "ldst") {
      print(S(1));
    } else if (op == "small") {
      print(eg::u256_small(word(t.at(1))));
    } else if (op == "zero") {
      print(eg::u256_zero());
    } else if (op == "eq") {
      std::printf("%d", eg::eq256(S(1), S(2)) ? 1 : 0);
    } else if (op == "lt") {
      std::printf("%d", eg::lt256(S(1), S(2)) ? 1 : 0);
    } else if (op == "sel") {
      print(eg::sel256(word(t.at(1)), S(2), S(3)));
    } else if (op == "add") {
      U256 a = S(1);
      const uint32_t carry = eg::add256(a, S(2));
      print(a);
      std::printf(" %u", carry);
    } else if (op == "sub") {
      U256 a = S(1);
      const uint32_t borrow = eg::sub256(a, S(2));
      print(a);
      std::printf(" %u", borrow);
    } else if (op == "addmod") {
      print(eg::addmod256(S(1), S(2), S(3)));
    } else if (op == "submod") {
      print(eg::submod256(S(1), S(2), S(3)));
    } else if (op == "negmod") {
      print(eg::negmod(S(1), S(2)));
    } else if (op == "mulsmall") {
      print(eg::mulsmall_mod(S(1), word(t.at(2)), S(3)));
    } else if (op == "mulmod") {
      print(eg::mulmod256(S(1), S(2), S(3)));
    } else if (op == "mulbyte") {
      print(eg::mulbyte_mod(S(1), word(t.at(2)), S(3)));
    } else if (op == "modany") {
      print(eg::mod256_any(S(1), S(2)));
    } else {
      std::fprintf(stderr, "unknown op %s\n", op.c_str());
      return 2;
    }
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}
