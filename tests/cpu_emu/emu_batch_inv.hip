// emu_batch_inv.hip — TEST-ONLY host build of K1b's block hand-off arithmetic
// (go-txflow_amd/csrc/fe_batch_inv.h): the very same __host__ __device__ fe_invert_each the kernel
// runs over its waves' running products, here over plain arrays.  It is not linked into
// libtxvote.so and the product never calls it.
#include "../../go-txflow_amd/csrc/fe_batch_inv.h"
#include "../../go-txflow_amd/csrc/fe_inv_var.h"

using namespace txv;

namespace {
struct HostChain {
  fe* xs;
  fe ps[8];
  fe x(int i) const { return xs[i]; }
  void set_x(int i, const fe& v) { xs[i] = v; }
  fe pre(int i) const { return ps[i]; }
  void set_pre(int i, const fe& v) { ps[i] = v; }
};
}  // namespace

// x: n elements of 8 words, replaced by their inverses (weakly reduced).  which 0: the divstep
// inverse K1b uses; 1: the Fermat chain.  Returns the number of calls of the inverter, -1 for a
// bad n.
extern "C" int emu_invert_each(uint32_t* x, int n, int which) {
  if (n < 1 || n > 8) return -1;
  HostChain m{reinterpret_cast<fe*>(x), {}};
  int calls = 0;
  fe_invert_each(m, n, [&](const fe& z) {
    ++calls;
    return which ? fe_invert(z) : fe_invert_var(z);
  });
  return calls;
}

// out = fe_invert(x) (the Fermat chain), canonical
extern "C" void emu_fe_invert_canon(const uint32_t* x, uint32_t* out) {
  fe z;
  for (int i = 0; i < 8; ++i) z.v[i] = x[i];
  const fe r = fe_canon(fe_invert(z));
  for (int i = 0; i < 8; ++i) out[i] = r.v[i];
}
