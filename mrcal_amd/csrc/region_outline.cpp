// The outline of the largest region of a mask: the definition is in include/mrcal_amd.h ("valid-intrinsics region").
//   1. the set cells are labelled by 8-connected component, in raster order of each component's first cell
//   2. from that first cell (the topmost, and the leftmost of its row) the outer border is followed from cell to cell:
//      at a cell that was entered by direction d, the neighbours are looked at clockwise beginning one past the way
//      back, (d + 4) + 1, and the first one that is set is the next cell. At the first cell the search begins at east.
//      The walk ends when it stands on the first cell and is about to repeat its first move; a component of one cell has
//      no move. A spur one cell wide is walked out and back
//   3. a cell of the walk is a vertex where the direction of leaving differs from that of arriving (the first cell
//      always is one)
//   4. twice the area: the shoelace sum over the vertices, its absolute value
// HOST code.
#include "region_outline.hpp"
#include <stdlib.h>

namespace mrcal_amd {

namespace {

// the border of the component that begins at (x0,y0) in raster order
std::vector<OutlineVertex> follow_border(const uint8_t* mask, int w, int h, int x0, int y0)
{
    auto set = [&](int x, int y) { return x >= 0 && x < w && y >= 0 && y < h && mask[(size_t)y*w + x] != 0; };
    std::vector<OutlineVertex> cells;      // the walk
    std::vector<int>           moves;      // moves[i]: from cells[i] to cells[i + 1] (cyclically)
    int x = x0, y = y0, search0 = 0, first_move = -1;
    const size_t limit = (size_t)8*w*h + 8;
    while(cells.size() < limit)
    {
        int move = -1;
        for(int k = 0; k < 8; k++)
        {
            const int d = (search0 + k) & 7;
            if(set(x + OUTLINE_DX[d], y + OUTLINE_DY[d])) { move = d; break; }
        }
        if(move < 0) { cells.push_back(OutlineVertex{ x, y }); break; }                     // one cell
        if(x == x0 && y == y0 && first_move >= 0 && move == first_move) break;              // around
        if(first_move < 0) first_move = move;
        cells.push_back(OutlineVertex{ x, y });
        moves.push_back(move);
        x += OUTLINE_DX[move];
        y += OUTLINE_DY[move];
        search0 = (move + 4 + 1) & 7;
    }
    if(moves.empty()) return cells;
    std::vector<OutlineVertex> vertices;
    const size_t n = cells.size();
    for(size_t i = 0; i < n; i++)
        if(moves[(i + n - 1) % n] != moves[i]) vertices.push_back(cells[i]);
    return vertices;
}

int64_t shoelace2(const std::vector<OutlineVertex>& v)
{
    int64_t a = 0;
    const size_t n = v.size();
    for(size_t i = 0; i < n; i++)
    {
        const OutlineVertex &p = v[i], &q = v[(i + 1) % n];
        a += (int64_t)p.x*q.y - (int64_t)q.x*p.y;
    }
    return a < 0 ? -a : a;
}

} // namespace

std::vector<OutlineVertex> region_outline(const uint8_t* mask, int w, int h, int64_t* area2)
{
    std::vector<OutlineVertex> best;
    int64_t best_area2 = -1;
    std::vector<uint8_t> seen((size_t)w*h, 0);
    std::vector<int> stack;
    for(int y0 = 0; y0 < h; y0++)
        for(int x0 = 0; x0 < w; x0++)
        {
            const size_t i0 = (size_t)y0*w + x0;
            if(mask[i0] == 0 || seen[i0]) continue;
            // (a new component: (x0,y0) is its first cell in raster order. Mark all of it)
            seen[i0] = 1;
            stack.push_back((int)i0);
            while(!stack.empty())
            {
                const int i = stack.back();
                stack.pop_back();
                const int x = i % w, y = i / w;
                for(int d = 0; d < 8; d++)
                {
                    const int xn = x + OUTLINE_DX[d], yn = y + OUTLINE_DY[d];
                    if(xn < 0 || xn >= w || yn < 0 || yn >= h) continue;
                    const size_t in = (size_t)yn*w + xn;
                    if(mask[in] == 0 || seen[in]) continue;
                    seen[in] = 1;
                    stack.push_back((int)in);
                }
            }
            std::vector<OutlineVertex> v = follow_border(mask, w, h, x0, y0);
            const int64_t a2 = shoelace2(v);
            if(a2 > best_area2) { best_area2 = a2; best.swap(v); }
        }
    if(area2) *area2 = best_area2 < 0 ? 0 : best_area2;
    return best;
}

} // namespace mrcal_amd

extern "C" int mrcal_amd_region_outline(const uint8_t* mask, int gridn_width, int gridn_height, int32_t* vertices, int capacity,
                                        int64_t* area2)
{
    if(mask == NULL || gridn_width <= 0 || gridn_height <= 0 || (int64_t)gridn_width*gridn_height > (int64_t)1 << 26 ||
       capacity < 0 || (capacity > 0 && vertices == NULL))
        return -1;
    const std::vector<mrcal_amd::OutlineVertex> v = mrcal_amd::region_outline(mask, gridn_width, gridn_height, area2);
    for(size_t i = 0; i < v.size() && (int)i < capacity; i++) { vertices[2*i] = v[i].x; vertices[2*i + 1] = v[i].y; }
    return (int)v.size();
}
