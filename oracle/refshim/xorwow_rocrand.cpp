// refshim/xorwow_rocrand.cpp -- the XORWOW recurrence and its jump-ahead for the shim's curand_init / curand,
// taken from rocRAND's host engine (third party, independent of the oracle's restatement).  Compiled as HIP host
// code only; there is no device code here.
#include <hip/hip_runtime.h>
#include <rocrand/rocrand_xorwow.h>

namespace {
struct Engine : public rocrand_device::xorwow_engine {
    void set(const unsigned int *v, unsigned int d) {
        for (int i = 0; i < 5; i++) m_state.x[i] = v[i];
        m_state.d = d;
    }
    void get(unsigned int *v, unsigned int *d) const {
        for (int i = 0; i < 5; i++) v[i] = m_state.x[i];
        *d = m_state.d;
    }
};
}  // namespace

extern "C" void mort_refshim_xorwow_skip(unsigned int *d, unsigned int *v, unsigned long long subsequence,
                                         unsigned long long offset) {
    Engine e;
    e.set(v, *d);
    e.discard_subsequence(subsequence);
    e.discard(offset);
    e.get(v, d);
}

extern "C" unsigned int mort_refshim_xorwow_next(unsigned int *d, unsigned int *v) {
    Engine e;
    e.set(v, *d);
    const unsigned int r = e.next();
    e.get(v, d);
    return r;
}
