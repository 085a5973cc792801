// fe_batch_inv.h — the inverses of n field elements from ONE inversion (Montgomery's trick) over
// elements that live behind an accessor, so K1b's block hand-off (kernels_verify.hip: the elements
// are the running products of a block's waves, in LDS) and the host build under tests/cpu_emu run
// the same code.
#pragma once
#include "fe.h"

namespace txv {

// x_i <- 1 / x_i for i < n (n >= 1): the prefix products c_i = x_0 ... x_i go to the accessor's
// scratch, inv runs once on c_{n-1}, and the walk back gives 1/x_i = u c_{i-1}, u <- u x_i.
// One inversion and 3 (n - 1) multiplies; the results are weakly reduced (fe.h), like fe_mul's.
//   M:   fe x(int i), void set_x(int i, const fe&), fe pre(int i), void set_pre(int i, const fe&)
//        (pre holds n - 1 elements)
//   Inv: fe operator()(const fe&), any exact inverse mod p
// No x_i may be 0 mod p, and there is deliberately no fallback for one: a zero would make every
// 1/x_i of the chain zero instead of only its own.  K1b's elements are products of Z coordinates
// of complete HWCD additions (never 0 on edwards25519) and the 1 of idle lanes; a fallback that
// patched a zero would turn a wrong Z into a verdict instead of leaving it visible.
template <class M, class Inv>
TXV_HD void fe_invert_each(M& m, int n, Inv inv) {
  fe c = m.x(0);
#pragma unroll 1
  for (int i = 1; i < n; ++i) {
    m.set_pre(i - 1, c);
    c = fe_mul(c, m.x(i));
  }
  fe u = inv(c);
#pragma unroll 1
  for (int i = n - 1; i > 0; --i) {
    const fe xi = m.x(i);
    m.set_x(i, fe_mul(u, m.pre(i - 1)));
    u = fe_mul(u, xi);
  }
  m.set_x(0, u);
}

}  // namespace txv
