/* CPU restatement of devmath.hpp sincos_lean (same constants, same fmas, same operation order) against sinl / cosl, per decade of
 * |x|: random magnitudes and the neighbours of multiples of pi/2. Prints the worst absolute error of the routine as it is
 * (quadrant from n in floating point) and as it was (quadrant from (int)n, out of range for |x| >= 2^31 * pi/2).
 *
 *   gcc -O2 -ffp-contract=off -mfma -o sincos_lean_restate tools/sincos_lean_restate.c -lm && ./sincos_lean_restate
 *
 * The figures in the header comment of sincos_lean and in DESIGN.md §5 "Off the fast paths" come from this program. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform01(void) {  /* xorshift64*, 53 bits */
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) * 0x1p-53;
}

static void sincos_lean(double x, double* s, double* c, int int_quadrant) {
  const double n = rint(x * 6.36619772367581382433e-01);
  double r = fma(-n, 1.57079632673412561417e+00, x);
  r = fma(-n, 6.07710050650619224932e-11, r);
  int q;
  if (int_quadrant) {  /* the former form; the device's conversion saturates, C's is undefined out of range: saturate by hand */
    q = n >= 2147483647.0 ? 2147483647 : (n <= -2147483648.0 ? (-2147483647 - 1) : (int)n);
  } else {
    q = (int)fma(-4.0, floor(n * 0.25), n);
  }
  const double z = r * r;
  double ps = fma(1.58969099521155010221e-10, z, -2.50507602534068634195e-08);
  ps = fma(ps, z, 2.75573137070700676789e-06);
  ps = fma(ps, z, -1.98412698298579493134e-04);
  ps = fma(ps, z, 8.33333333332248946124e-03);
  ps = fma(ps, z, -1.66666666666666324348e-01);
  const double sr = fma(ps * z, r, r);
  double pc = fma(-1.13596475577881948265e-11, z, 2.08757232129817482790e-09);
  pc = fma(pc, z, -2.75573143513906633035e-07);
  pc = fma(pc, z, 2.48015872894767294178e-05);
  pc = fma(pc, z, -1.38888888888741095749e-03);
  pc = fma(pc, z, 4.16666666666666019037e-02);
  const double hz = 0.5 * z;
  const double a = 1.0 - hz;
  const double cr = a + (((1.0 - a) - hz) + z * (z * pc));
  const double s0 = (q & 1) ? cr : sr;
  const double c0 = (q & 1) ? sr : cr;
  *s = (q & 2) ? -s0 : s0;
  *c = ((q + 1) & 2) ? -c0 : c0;
}

static double worst[2];
static void point(double x) {
  const long double ws = sinl((long double)x), wc = cosl((long double)x);
  for (int v = 0; v < 2; ++v) {
    double s, c;
    sincos_lean(x, &s, &c, v);
    const double es = (double)fabsl((long double)s - ws), ec = (double)fabsl((long double)c - wc);
    if (es > worst[v]) worst[v] = es;
    if (ec > worst[v]) worst[v] = ec;
  }
}

int main(void) {
  const long double half_pi = 1.57079632679489661923132169163975144L;
  printf("long double epsilon %.3Lg\n", (long double)__LDBL_EPSILON__);
  printf("%-22s %-14s %-14s\n", "|x| in", "float quadrant", "int quadrant");
  const double edges[] = {0.0, 1.0, 10.0, 1e2, 1e3, 1e4, 1e5, 1e6, 1.6e6, 1e7, 1e8, 1e9, 3.3e9, 3.4e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15};
  for (unsigned d = 0; d + 1 < sizeof(edges) / sizeof(edges[0]); ++d) {
    const double lo = edges[d], hi = edges[d + 1];
    worst[0] = worst[1] = 0.0;
    for (int i = 0; i < 2000000; ++i) {
      const double u = uniform01();
      const double m = lo > 0.0 ? lo * pow(hi / lo, u) : hi * u;
      const double x = (i & 1) ? -m : m;
      point(x);
      if ((i & 3) == 0) {  /* the multiple of pi/2 nearest to x and both neighbours */
        const double k = (double)(rintl((long double)x / half_pi) * half_pi);
        point(k);
        point(nextafter(k, INFINITY));
        point(nextafter(k, -INFINITY));
      }
    }
    printf("[%-8g, %-8g]   %-14.3g %-14.3g\n", lo, hi, worst[0], worst[1]);
  }
  return 0;
}
