// Stand-alone driver of every function of zkp_amd/csrc/sc25519.h on the host, built with g++ -fsanitize=address,undefined by
// tests/test_host_sc_onepass.py.  The header is one text for g++ and hipcc, so what runs here is what the kernels compile.
//
//   argv[1]: a file of records, one per line: "<op> <a> <b> <c>", op decimal, a / b / c 64 hex digits (256-bit values, little-endian bytes)
//   stdout:  one line per record, 64-hex-digit fields separated by blanks
//
//   op  0 sc_reduce(a)            1 sc_to_mont(a)             2 sc_mont(a, b)           3 sc_mul(a, b)          4 sc_muladd(a, b, c)
//       5 sc_mul_u128(a, b[0..4)) 6 sc_add(a, b)              7 sc_neg(a)               8 sc_from_wide(a, b)    9 sc_halve(a)
//      10 sc_halve_canonical(a)  11 sc_invert(a)             12 sc_fold_sign(a): s, flag              13 sc_not_canonical(a): flag
//      14 sc_cond_sub_l(a)       15 sc_add_pattern(a, b[0]): e, top        16 sc_reduce_384(a || b[0..4))          17 sc_reduce_wide(a || b)
//      18 sc_sqmul(y = a, n = c[0] & 7, t = b)                19 sc_muladd, r aliasing a        20 sc_mul, r aliasing b
//      21 sc_reduce_tail(a || c[0] as limb 8)
// The caller keeps each function's preconditions (which operand must be below l, or below 2 l, or below 67 * 2^252).
#include "../../zkp_amd/csrc/sc25519.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace zkp;

static bool hex32(const char* s, uint32_t v[8]) {
  uint8_t b[32];
  for (int i = 0; i < 32; ++i) {
    unsigned x;
    if (sscanf(s + 2 * i, "%2x", &x) != 1) return false;
    b[i] = (uint8_t)x;
  }
  memcpy(v, b, 32);
  return true;
}
static void put(const uint32_t v[8]) {
  uint8_t b[32];
  memcpy(b, v, 32);
  for (int i = 0; i < 32; ++i) printf("%02x", b[i]);
}
static void put_word(uint32_t w) {
  uint32_t v[8] = {w, 0, 0, 0, 0, 0, 0, 0};
  put(v);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char* line = static_cast<char*>(malloc(512));
  size_t n = 0;
  while (fgets(line, 512, f)) {
    int op, used = 0;
    if (sscanf(line, "%d %n", &op, &used) != 1 || strlen(line + used) < 3 * 64 + 2) continue;
    // every operand on the heap in a block of exactly its size: an access past a limb array shows under AddressSanitizer
    sc* a = static_cast<sc*>(malloc(sizeof(sc)));
    sc* b = static_cast<sc*>(malloc(sizeof(sc)));
    sc* c = static_cast<sc*>(malloc(sizeof(sc)));
    sc* r = static_cast<sc*>(malloc(sizeof(sc)));
    if (!hex32(line + used, a->v) || !hex32(line + used + 65, b->v) || !hex32(line + used + 130, c->v)) return 2;
    sc_zero(*r);
    switch (op) {
      case 0: sc_reduce(*r, *a); put(r->v); break;
      case 1: sc_to_mont(*r, *a); put(r->v); break;
      case 2: sc_mont(*r, *a, *b); put(r->v); break;
      case 3: sc_mul(*r, *a, *b); put(r->v); break;
      case 4: sc_muladd(*r, *a, *b, *c); put(r->v); break;
      case 5: {
        uint32_t* w = static_cast<uint32_t*>(malloc(16));
        memcpy(w, b->v, 16);
        sc_mul_u128(*r, *a, w);
        free(w);
        put(r->v);
        break;
      }
      case 6: sc_add(*r, *a, *b); put(r->v); break;
      case 7: sc_neg(*r, *a); put(r->v); break;
      case 8: sc_from_wide(*r, *a, *b); put(r->v); break;
      case 9: sc_halve(*r, *a); put(r->v); break;
      case 10: sc_halve_canonical(*r, *a); put(r->v); break;
      case 11: sc_invert(*r, *a); put(r->v); break;
      case 12: {
        const uint32_t flag = sc_fold_sign(a->v);
        put(a->v); putchar(' '); put_word(flag);
        break;
      }
      case 13: put_word(sc_not_canonical(a->v)); break;
      case 14: sc_cond_sub_l(*a); put(a->v); break;
      case 15: {
        uint32_t top;
        sc_add_pattern(r->v, top, a->v, b->v[0]);
        put(r->v); putchar(' '); put_word(top);
        break;
      }
      case 16: {
        uint32_t* x = static_cast<uint32_t*>(malloc(48));
        memcpy(x, a->v, 32);
        memcpy(x + 8, b->v, 16);
        sc_reduce_384(*r, x);
        free(x);
        put(r->v);
        break;
      }
      case 17: {
        uint32_t* x = static_cast<uint32_t*>(malloc(64));
        memcpy(x, a->v, 32);
        memcpy(x + 8, b->v, 32);
        sc_reduce_wide(*r, x);
        free(x);
        put(r->v);
        break;
      }
      case 18: sc_sqmul(*a, (int)(c->v[0] & 7u), *b); put(a->v); break;
      case 19: sc_muladd(*a, *a, *b, *c); put(a->v); break;
      case 20: sc_mul(*b, *a, *b); put(b->v); break;
      case 21: {
        uint32_t* x = static_cast<uint32_t*>(malloc(36));
        memcpy(x, a->v, 32);
        x[8] = c->v[0];
        sc_reduce_tail(*r, x);
        free(x);
        put(r->v);
        break;
      }
      default: return 2;
    }
    putchar('\n');
    free(a); free(b); free(c); free(r);
    ++n;
  }
  free(line);
  fclose(f);
  return n ? 0 : 2;
}
