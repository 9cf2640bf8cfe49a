// Part e of "chessboard corners" (include/mrcal_amd.h): the lattice among the refined candidates. HOST code.
//
//   neighbours   the candidates lie in a uniform bucket grid of about two to a cell; the K nearest of a candidate come
//                from the rings of cells around its own, so that 4096 candidates cost no 4096^2
//   seeds        in descending response. A seed c needs two pairs of opposite neighbours (a,b),
//                |a + b - 2c| <= 0.25 min(|a-c|, |b-c|), that are not parallel: the shortest pair, and the shortest pair
//                more than asin(0.3) off it. They are the lattice's +-i and +-j at c, if the four cells diagonally across
//                are found where these predict them: a seed is the middle of a 3 x 3 patch
//   growth       over lattice cells, in passes until one assigns nothing. The cell past (cell) from (previous) is
//                predicted at 2 p(cell) - p(previous); with no previous cell, at p(cell) + the parallel edge of a
//                neighbouring row. The nearest unassigned candidate within 0.3 of that step's length is taken
//   acceptance   rows and columns at the rim that are not full are peeled off, the emptiest first (what grew into
//                clutter next to the board goes this way); what is left must be exactly the full W x H or H x W rectangle. Otherwise the
//                next seed that was in no failed lattice is tried
//   orientation  of the proper labellings the one whose mean +i edge points most along +x
#include <math.h>
#include <stddef.h>
#include <algorithm>
#include <vector>
#include "chessboard_grid.hpp"

namespace mrcal_amd {

namespace {

struct P2 { double x, y; };
inline P2     operator+(P2 a, P2 b) { return P2{ a.x + b.x, a.y + b.y }; }
inline P2     operator-(P2 a, P2 b) { return P2{ a.x - b.x, a.y - b.y }; }
inline double norm(P2 a)            { return sqrt(a.x*a.x + a.y*a.y); }
inline double cross(P2 a, P2 b)     { return a.x*b.y - a.y*b.x; }

const int    NEIGHBOURS    = 12;
const double PAIR_SYMMETRY = 0.25;      // |a + b - 2c| over the shorter arm
const double PAIR_PARALLEL = 0.3;       // |sin| of the angle below which two pairs are one direction
const double GROW_RADIUS   = 0.3;       // of the step's length

struct Buckets
{
    const std::vector<P2>& p;
    double x0 = 0., y0 = 0., cell = 1.;
    int    nx = 1, ny = 1;
    std::vector<int> start, items;      // the points of cell k: items[start[k] .. start[k+1])

    explicit Buckets(const std::vector<P2>& points) : p(points)
    {
        const int n = (int)p.size();
        double x1 = 0., y1 = 0.;
        for(int i=0;i<n;i++)
        {
            if(i == 0 || p[i].x < x0) x0 = p[i].x;
            if(i == 0 || p[i].y < y0) y0 = p[i].y;
            if(i == 0 || p[i].x > x1) x1 = p[i].x;
            if(i == 0 || p[i].y > y1) y1 = p[i].y;
        }
        const double w = x1 - x0, h = y1 - y0;
        cell = sqrt(2.*(w*h > 1. ? w*h : 1.)/(n > 0 ? n : 1));
        if(cell < (w > h ? w : h)/512.) cell = (w > h ? w : h)/512.;
        nx = (int)(w/cell) + 1; ny = (int)(h/cell) + 1;
        start.assign((size_t)nx*ny + 1, 0);
        for(int i=0;i<n;i++) start[cell_of(p[i]) + 1]++;
        for(size_t k=0;k<(size_t)nx*ny;k++) start[k+1] += start[k];
        items.assign(n, 0);
        std::vector<int> at(start.begin(), start.end() - 1);
        for(int i=0;i<n;i++) items[at[cell_of(p[i])]++] = i;
    }
    int cx_of(double x) const { const int c = (int)floor((x - x0)/cell); return c < 0 ? 0 : c >= nx ? nx - 1 : c; }
    int cy_of(double y) const { const int c = (int)floor((y - y0)/cell); return c < 0 ? 0 : c >= ny ? ny - 1 : c; }
    int cell_of(P2 a)  const { return cy_of(a.y)*nx + cx_of(a.x); }

    // the K nearest other points of point c, nearest first
    void nearest(std::vector<int>* out, int c, int K) const
    {
        std::vector<std::pair<double,int>> found;
        const int cx = cx_of(p[c].x), cy = cy_of(p[c].y);
        const int rings = nx > ny ? nx : ny;
        for(int r=0; r<=rings; r++)
        {
            for(int y=cy-r; y<=cy+r; y++)
            {
                if(y < 0 || y >= ny) continue;
                const int dx = (y == cy - r || y == cy + r) ? 1 : 2*r;
                for(int x=cx-r; x<=cx+r; x+=(dx > 0 ? dx : 1))
                {
                    if(x < 0 || x >= nx) continue;
                    for(int k=start[y*nx + x]; k<start[y*nx + x + 1]; k++)
                        if(items[k] != c) found.push_back({ norm(p[items[k]] - p[c]), items[k] });
                }
            }
            // (every point of a ring not yet looked at is farther than r cells)
            if((int)found.size() >= K)
            {
                std::sort(found.begin(), found.end());
                if(found[K - 1].first <= r*cell) break;
            }
        }
        std::sort(found.begin(), found.end());
        out->clear();
        for(int k=0; k<K && k<(int)found.size(); k++) out->push_back(found[k].second);
    }

    // the nearest point to `at` within `radius` that is not taken; -1: none
    int nearest_free(P2 at, double radius, const std::vector<char>& taken) const
    {
        if(!(radius > 0.) || !isfinite(at.x) || !isfinite(at.y)) return -1;
        if(at.x + radius < x0 || at.y + radius < y0 || at.x - radius > x0 + nx*cell || at.y - radius > y0 + ny*cell) return -1;
        int best = -1;
        double dbest = radius;
        for(int y=cy_of(at.y - radius); y<=cy_of(at.y + radius); y++)
            for(int x=cx_of(at.x - radius); x<=cx_of(at.x + radius); x++)
                for(int k=start[y*nx + x]; k<start[y*nx + x + 1]; k++)
                {
                    const int i = items[k];
                    if(taken[i]) continue;
                    const double d = norm(p[i] - at);
                    if(d < dbest || (d == dbest && best >= 0 && i < best) || (d == dbest && best < 0)) { dbest = d; best = i; }
                }
        return best;
    }
};

struct Lattice
{
    int M, S;                           // cells -M..M a side: S = 2M + 1
    std::vector<int> at;                // the point of a cell, -1: none
    std::vector<std::pair<int,int>> cells;
    explicit Lattice(int m) : M(m), S(2*m + 1), at((size_t)(2*m + 1)*(2*m + 1), -1) {}
    bool inside(int i, int j) const { return i >= -M && i <= M && j >= -M && j <= M; }
    int& operator()(int i, int j)       { return at[(size_t)(j + M)*S + (i + M)]; }
    int  get(int i, int j) const        { return inside(i, j) ? at[(size_t)(j + M)*S + (i + M)] : -1; }
};

// the two pairs of opposite neighbours of seed c: i1 - c - i0 and j1 - c - j0
bool seed_axes(int* i0, int* i1, int* j0, int* j1, int c, const std::vector<P2>& p, const std::vector<int>& nb)
{
    struct Pair { double length; int a, b; P2 dir; };
    std::vector<Pair> pairs;
    for(size_t ia=0; ia<nb.size(); ia++)
        for(size_t ib=ia+1; ib<nb.size(); ib++)
        {
            const P2 a = p[nb[ia]] - p[c], b = p[nb[ib]] - p[c];
            const double la = norm(a), lb = norm(b);
            if(!(la > 0. && lb > 0.)) continue;
            if(norm(a + b) <= PAIR_SYMMETRY*(la < lb ? la : lb))
            {
                const P2 d = a - b;
                const double ld = norm(d);
                pairs.push_back(Pair{ (la + lb)/2., nb[ia], nb[ib], P2{ d.x/ld, d.y/ld } });
            }
        }
    if(pairs.size() < 2) return false;
    std::stable_sort(pairs.begin(), pairs.end(), [](const Pair& u, const Pair& v) { return u.length < v.length; });
    for(size_t k=1; k<pairs.size(); k++)
        if(fabs(cross(pairs[0].dir, pairs[k].dir)) > PAIR_PARALLEL)
        {
            *i1 = pairs[0].a; *i0 = pairs[0].b; *j1 = pairs[k].a; *j0 = pairs[k].b;
            return *i0 != *j0 && *i0 != *j1 && *i1 != *j0 && *i1 != *j1;
        }
    return false;
}

void grow(Lattice* L, std::vector<char>* taken, const std::vector<P2>& p, const Buckets& buckets)
{
    static const int DIR[4][2] = { {1,0}, {-1,0}, {0,1}, {0,-1} };
    bool changed = true;
    while(changed)
    {
        changed = false;
        for(size_t k=0; k<L->cells.size(); k++)
        {
            const int i = L->cells[k].first, j = L->cells[k].second;
            const P2 here = p[L->get(i, j)];
            for(const int* d : DIR)
            {
                const int ti = i + d[0], tj = j + d[1];
                if(!L->inside(ti, tj) || L->get(ti, tj) >= 0) continue;
                P2 step;
                const int previous = L->get(i - d[0], j - d[1]);
                if(previous >= 0) step = here - p[previous];
                else
                {
                    // the parallel edge of a neighbouring row: across d
                    int n1 = L->get(i + d[1], j + d[0]), n2 = L->get(i + d[1] + d[0], j + d[0] + d[1]);
                    if(n1 < 0 || n2 < 0) { n1 = L->get(i - d[1], j - d[0]); n2 = L->get(i - d[1] + d[0], j - d[0] + d[1]); }
                    if(n1 < 0 || n2 < 0) continue;
                    step = p[n2] - p[n1];
                }
                const int found = buckets.nearest_free(here + step, GROW_RADIUS*norm(step), *taken);
                if(found < 0) continue;
                (*L)(ti, tj) = found;
                (*taken)[found] = 1;
                L->cells.push_back({ ti, tj });
                changed = true;
            }
        }
    }
}

// peels the rows and columns at the rim that are not full; the box that is left
void peel(Lattice* L, int* imin, int* imax, int* jmin, int* jmax)
{
    *imin = *jmin = L->M + 1; *imax = *jmax = -L->M - 1;
    for(const auto& c : L->cells)
    {
        *imin = std::min(*imin, c.first);  *imax = std::max(*imax, c.first);
        *jmin = std::min(*jmin, c.second); *jmax = std::max(*jmax, c.second);
    }
    // one line at a time, the emptiest first: a stray cell next to the board lengthens the lines across it, which
    // are then one short of full and must outlast it
    while(*imin <= *imax && *jmin <= *jmax)
    {
        int    worst = -1;
        double worst_fill = 1.;
        for(int side=0; side<4; side++)
        {
            const bool column = side < 2;
            const int  line   = side == 0 ? *imin : side == 1 ? *imax : side == 2 ? *jmin : *jmax;
            const int  lo     = column ? *jmin : *imin, hi = column ? *jmax : *imax;
            int n = 0;
            for(int k=lo; k<=hi; k++) n += (column ? L->get(line, k) : L->get(k, line)) >= 0;
            const double fill = (double)n/(hi - lo + 1);
            if(fill < worst_fill) { worst_fill = fill; worst = side; }
        }
        if(worst < 0) break;
        const bool column = worst < 2;
        const int  line   = worst == 0 ? *imin : worst == 1 ? *imax : worst == 2 ? *jmin : *jmax;
        const int  lo     = column ? *jmin : *imin, hi = column ? *jmax : *imax;
        for(int k=lo; k<=hi; k++) { if(column) (*L)(line, k) = -1; else (*L)(k, line) = -1; }
        if(worst == 0) ++*imin; else if(worst == 1) --*imax; else if(worst == 2) ++*jmin; else --*jmax;
    }
}

} // namespace

bool chessboard_grid(int N, const double* q, const int32_t* response, const int32_t* status,
                     int board_width, int board_height, double* corners)
{
    const int W = board_width, H = board_height;
    if(W < 3 || H < 3 || N < W*H) return false;
    std::vector<P2>  p;
    std::vector<int> order;             // into p, the seeds in the order they are tried
    {
        std::vector<std::pair<long,int>> by_response;
        for(int i=0;i<N;i++)
        {
            if(status != NULL && status[i] != 0) continue;
            if(!isfinite(q[2*i]) || !isfinite(q[2*i+1])) continue;
            by_response.push_back({ response != NULL ? -(long)response[i] : 0L, (int)p.size() });
            p.push_back(P2{ q[2*i], q[2*i+1] });
        }
        std::stable_sort(by_response.begin(), by_response.end());
        for(const auto& s : by_response) order.push_back(s.second);
    }
    const int n = (int)p.size();
    if(n < W*H) return false;
    const Buckets buckets(p);
    std::vector<char> failed(n, 0);
    std::vector<int>  nb;
    for(int seed : order)
    {
        if(failed[seed]) continue;
        buckets.nearest(&nb, seed, NEIGHBOURS);
        int i0, i1, j0, j1;
        if(!seed_axes(&i0, &i1, &j0, &j1, seed, p, nb)) continue;
        // the four cells diagonally across must be there too: two pairs that are the lattice's axes have them, a pair
        // made of clutter, or a seed at the rim, does not
        std::vector<char> taken(n, 0);
        bool patch = true;
        for(int a : { i0, i1 }) for(int b : { j0, j1 })
        {
            const double la = norm(p[a] - p[seed]), lb = norm(p[b] - p[seed]);
            if(buckets.nearest_free(p[a] + p[b] - p[seed], GROW_RADIUS*(la < lb ? la : lb), taken) < 0) patch = false;
        }
        if(!patch) continue;
        Lattice L(W > H ? W : H);
        const int first[5][3] = { {0,0,seed}, {1,0,i1}, {-1,0,i0}, {0,1,j1}, {0,-1,j0} };
        for(const int* f : first) { L(f[0], f[1]) = f[2]; taken[f[2]] = 1; L.cells.push_back({ f[0], f[1] }); }
        grow(&L, &taken, p, buckets);
        for(int i=0;i<n;i++) if(taken[i]) failed[i] = 1;        // (if this is the board, nothing more is tried)

        int imin, imax, jmin, jmax;
        peel(&L, &imin, &imax, &jmin, &jmax);
        const int bw = imax - imin + 1, bh = jmax - jmin + 1;
        if(!((bw == W && bh == H) || (bw == H && bh == W))) continue;
        bool full = true;
        for(int j=jmin; j<=jmax && full; j++) for(int i=imin; i<=imax; i++) if(L.get(i, j) < 0) { full = false; break; }
        if(!full) continue;

        // the labellings: label (ii,jj) is cell (a,b) = (ii,jj), or (jj,ii) transposed, either axis flipped
        double best = 0.;
        int    best_t = -1, best_fi = 0, best_fj = 0;
        auto point = [&](int t, int fi, int fj, int ii, int jj) -> P2
        {
            int a = t ? jj : ii, b = t ? ii : jj;
            if(fi) a = bw - 1 - a;
            if(fj) b = bh - 1 - b;
            return p[L.get(imin + a, jmin + b)];
        };
        for(int t=0; t<2; t++)
        {
            if(t == 0 ? !(bw == W && bh == H) : !(bw == H && bh == W)) continue;
            for(int fi=0; fi<2; fi++) for(int fj=0; fj<2; fj++)
            {
                P2 ei{ 0., 0. }, ej{ 0., 0. };
                for(int jj=0; jj<H; jj++) for(int ii=0; ii+1<W; ii++) ei = ei + (point(t, fi, fj, ii+1, jj) - point(t, fi, fj, ii, jj));
                for(int jj=0; jj+1<H; jj++) for(int ii=0; ii<W; ii++) ej = ej + (point(t, fi, fj, ii, jj+1) - point(t, fi, fj, ii, jj));
                if(!(cross(ei, ej) > 0.)) continue;
                const double x = ei.x/norm(ei);
                if(best_t < 0 || x > best) { best = x; best_t = t; best_fi = fi; best_fj = fj; }
            }
        }
        if(best_t < 0) continue;
        for(int jj=0; jj<H; jj++) for(int ii=0; ii<W; ii++)
        {
            const P2 c = point(best_t, best_fi, best_fj, ii, jj);
            corners[2*(jj*W + ii)] = c.x; corners[2*(jj*W + ii) + 1] = c.y;
        }
        return true;
    }
    return false;
}

} // namespace mrcal_amd
