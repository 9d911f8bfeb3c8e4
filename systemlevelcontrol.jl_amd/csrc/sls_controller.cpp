// sls_controller.cpp — host twin of the stand-alone controller step (pure C++, no HIP): the same tables (FirOperator), the
// same mirrored ring and β double buffer (sls_controller.h) as csrc/sls_controller.hip, one serial loop.  Reference of the
// non-GPU tests; the GPU tests hold the device to a long-double statement that shares no code with either.
#include "sls_controller.h"

#include <vector>

namespace sls {

int controller_host(const FirOperator& F, const double* values, int64_t nscen, int64_t steps, const double* x, double* u,
                    double* what, std::string& msg) {
  if (nscen < 1 || steps < 0) { msg = "nscen must be >= 1 and steps >= 0"; return SLS_EINVAL; }
  if (steps > 0 && !x) { msg = "null x"; return SLS_EINVAL; }
  const int64_t Nx = F.Nx, Nu = F.Nu, ns = nscen;
  if ((int64_t)F.beta_ptr.size() != Nx + 1 || (int64_t)F.u_ptr.size() != Nu + 1) { msg = "operator tables missing"; return SLS_EINVAL; }
  const int64_t nent = F.u_ptr[Nu];
  if (nent > 0 && !values) { msg = "null values"; return SLS_EINVAL; }
  const int64_t R = controller_ring_slots(F.T);
  std::vector<double> vals((size_t)nent);                              // the gather of sls_controller_load
  for (int64_t e = 0; e < nent; ++e) vals[e] = values[F.perm[e]];
  std::vector<double> hist((size_t)controller_hist_doubles(Nx, F.T, ns), 0.0), beta((size_t)controller_beta_doubles(Nx, ns), 0.0);
  for (int64_t k = 0; k < steps; ++k) {
    const int64_t s = controller_slot(k, R);
    const double* xk = x + k * Nx * ns;
    const double* bk = beta.data() + (k & 1) * Nx * ns;
    double* bn = beta.data() + ((k + 1) & 1) * Nx * ns;
    const double* win = hist.data() + controller_window_end(s, R, Nx) * ns;
    auto row = [&](int64_t beg, int64_t end, int64_t sc) {
      long double a = 0.0L;
      for (int64_t e = beg; e < end; ++e) {
        const int64_t h = F.hoff[e];
        const double w = h <= Nx ? xk[(Nx - h) * ns + sc] - bk[(Nx - h) * ns + sc] : win[-h * ns + sc];
        a += (long double)vals[e] * (long double)w;
      }
      return (double)a;
    };
    for (int64_t sc = 0; sc < ns; ++sc) {
      for (int64_t i = 0; i < Nx; ++i) bn[i * ns + sc] = row(F.beta_ptr[i], F.beta_ptr[i + 1], sc);
      for (int64_t j = 0; j < Nu; ++j) {
        const double uj = row(F.u_ptr[j], F.u_ptr[j + 1], sc);
        if (u) u[(k * Nu + j) * ns + sc] = uj;
      }
    }
    // ŵ_k into both copies of its slot, after every row has read the window (the device writes s and s + R, which no row reads)
    for (int64_t i = 0; i < Nx * ns; ++i) {
      const double w = xk[i] - bk[i];
      hist[(size_t)(s * Nx * ns + i)] = w;
      hist[(size_t)((s + R) * Nx * ns + i)] = w;
      if (what) what[k * Nx * ns + i] = w;
    }
  }
  return 0;
}

}  // namespace sls
