// Host build of mrcal_amd/csrc/triangulation_math.hpp for tests/test_triangulation.py: the same tri_eval() the
// kernel's lanes run, in a loop over the pairs. Built with -ffp-contract=on like the library
#include "../../mrcal_amd/csrc/triangulation_math.hpp"

using namespace mrcal_amd;

namespace {
template<int METHOD>
void eval_all(int with_grad, int N, const double* v0, const double* v1, const double* pose,
              double* p, double* g0, double* g1, double* gp)
{
    constexpr int NP = tri_pose_size(METHOD);
    for(int i=0;i<N;i++)
    {
        if(with_grad) tri_eval<METHOD, true,  3>(p + 3*i, g0 + 9*i, g1 + 9*i, gp + 3*NP*i, v0 + 3*i, v1 + 3*i, pose + NP*i);
        else          tri_eval<METHOD, false, 3>(p + 3*i, NULL, NULL, NULL,                v0 + 3*i, v1 + 3*i, pose + NP*i);
    }
}
}

extern "C" {

// method: TriMethod. 0 on success
int tricheck_eval(int method, int with_grad, int N, const double* v0, const double* v1, const double* pose,
                  double* p, double* g0, double* g1, double* gp)
{
    switch(method)
    {
    case TRI_GEOMETRIC:       eval_all<TRI_GEOMETRIC      >(with_grad, N, v0, v1, pose, p, g0, g1, gp); return 0;
    case TRI_LINDSTROM:       eval_all<TRI_LINDSTROM      >(with_grad, N, v0, v1, pose, p, g0, g1, gp); return 0;
    case TRI_LEECIVERA_L1:    eval_all<TRI_LEECIVERA_L1   >(with_grad, N, v0, v1, pose, p, g0, g1, gp); return 0;
    case TRI_LEECIVERA_LINF:  eval_all<TRI_LEECIVERA_LINF >(with_grad, N, v0, v1, pose, p, g0, g1, gp); return 0;
    case TRI_LEECIVERA_MID2:  eval_all<TRI_LEECIVERA_MID2 >(with_grad, N, v0, v1, pose, p, g0, g1, gp); return 0;
    case TRI_LEECIVERA_WMID2: eval_all<TRI_LEECIVERA_WMID2>(with_grad, N, v0, v1, pose, p, g0, g1, gp); return 0;
    }
    return 1;
}

// the methods on plain doubles (the header's other scalar): the point alone. 0 on success
int tricheck_eval_double(int method, int N, const double* v0, const double* v1, const double* pose, double* p)
{
    for(int i=0;i<N;i++)
    {
        double m[3] = {0., 0., 0.};
        bool ok;
        switch(method)
        {
        case TRI_GEOMETRIC:       ok = tri_geometric      (m, v0 + 3*i, v1 + 3*i, pose + 3*i);  break;
        case TRI_LINDSTROM:       ok = tri_lindstrom      (m, v0 + 3*i, v1 + 3*i, pose + 12*i); break;
        case TRI_LEECIVERA_L1:    ok = tri_leecivera_l1   (m, v0 + 3*i, v1 + 3*i, pose + 3*i);  break;
        case TRI_LEECIVERA_LINF:  ok = tri_leecivera_linf (m, v0 + 3*i, v1 + 3*i, pose + 3*i);  break;
        case TRI_LEECIVERA_MID2:  ok = tri_leecivera_mid2 (m, v0 + 3*i, v1 + 3*i, pose + 3*i);  break;
        case TRI_LEECIVERA_WMID2: ok = tri_leecivera_wmid2(m, v0 + 3*i, v1 + 3*i, pose + 3*i);  break;
        default: return 1;
        }
        for(int k=0;k<3;k++) p[3*i + k] = ok ? m[k] : 0.0;
    }
    return 0;
}

void tricheck_is_convergent(int N, const double* v0, const double* v1, const double* t01, int* out)
{
    for(int i=0;i<N;i++) out[i] = tri_leecivera_mid2_is_convergent(v0 + 3*i, v1 + 3*i, t01 + 3*i) ? 1 : 0;
}

}
