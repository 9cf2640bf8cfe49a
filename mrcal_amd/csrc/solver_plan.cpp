// The solver's work lists (solver_plan.hpp): which Gram position, which row, adds to which entry of the normal
// equations, and in which order.
#include <string.h>
#include <algorithm>
#include <unordered_map>
#include "host_state.hpp"
#include "solver_plan.hpp"

namespace mrcal_amd {

DestLists make_dest_lists(const DestSources& sources)
{
    DestLists d;
    d.begin.push_back(0);
    for(const auto& kv : sources)
    {
        d.id.push_back(kv.first);
        d.src.insert(d.src.end(), kv.second.begin(), kv.second.end());
        d.begin.push_back((int)d.src.size());
    }
    return d;
}

// The frame part of the Gram positions, per position and per observation (AssemblyPlan::frame_pos, obs_cols). Derived
// from pair_table and checked against it: every pair's operation at every position must come back out
static bool plan_frame_part(const DeviceProblem& D, const NormalDims& nd, const BoardObsMeta* meta,
                            const std::vector<int>& pair_rep, BoardGramPlan* plan)
{
    const int Nobs = D.Nobs_board, npos = (int)plan->pos_table.size();
    const std::vector<PairOp>& ptab = plan->pair_table;
    const int nintr = (D.Nintr_state > 0) ? D.Ncameras_intrinsics*D.Nintr_state : 0;
    std::vector<int>& fpos = plan->frame_pos;
    fpos.assign(npos, FRAMEPOS_NONE);
    std::vector<int> pair_cols(2*pair_rep.size(), -1);
    auto classify = [&](const PairOp& op, int* kind, int* a, int* k, int* base) -> void
    {
        *kind = FRAMEPOS_NONE; *a = 0; *k = 0; *base = -1;
        const int b = op.aux >> 16;
        switch(op.op & 0xff)
        {
        case PAIROP_D:  *kind = (op.op & PAIROP_MIRROR) ? FRAMEPOS_D_MIRROR : FRAMEPOS_D; *a = op.aux & 0xffff; *k = b; break;
        case PAIROP_GF: *kind = FRAMEPOS_GF; *a = op.aux & 0xffff; break;
        case PAIROP_BT:
            *a = op.aux & 0xffff;
            if(b < nintr)        { *kind = FRAMEPOS_BT_INTRINSICS; *base = (b/D.Nintr_state)*D.Nintr_state; *k = b - *base; }
            else if(b < nd.Nc - nd.Nwarp) { *kind = FRAMEPOS_BT_EXTRINSICS; *base = nintr + ((b - nintr)/6)*6;     *k = b - *base; }
            else                 { *kind = FRAMEPOS_BT_WARP; *k = b; }
            break;
        default: break;
        }
    };
    bool consistent = true;
    for(size_t ip = 0; ip < pair_rep.size(); ip++)
        for(int pos = 0; pos < npos; pos++)
        {
            int kind, a, k, base;
            classify(ptab[ip*npos + pos], &kind, &a, &k, &base);
            if(kind == FRAMEPOS_NONE) continue;
            const int code = kind | (a << 3) | (k << 6);
            if(fpos[pos] == FRAMEPOS_NONE) fpos[pos] = code;
            else if(fpos[pos] != code) consistent = false;
            if(kind == FRAMEPOS_BT_INTRINSICS || kind == FRAMEPOS_BT_EXTRINSICS)
            {
                int& c = pair_cols[2*ip + (kind == FRAMEPOS_BT_EXTRINSICS ? 1 : 0)];
                if(c < 0) c = base; else if(c != base) consistent = false;
            }
        }
    // ... and back: a pair without a block (the camera at the reference has no extrinsics) has nothing
    // at that block's positions, and every other position reads the same through both tables
    for(size_t ip = 0; ip < pair_rep.size() && consistent; ip++)
        for(int pos = 0; pos < npos; pos++)
        {
            // (observations without an eliminated pose - a camera at the reference, with elim_extrinsics -
            //  are in no block's list: what the frame part's tables say about them is never looked at)
            const BoardObsMeta& m = meta[pair_rep[ip]];
            if((nd.elim_extrinsics ? m.icam_extrinsics : m.iframe) < 0) break;
            int kind, a, k, base;
            classify(ptab[ip*npos + pos], &kind, &a, &k, &base);
            const int fk = fpos[pos] & 7;
            const bool absent = (fk == FRAMEPOS_BT_INTRINSICS && pair_cols[2*ip] < 0) || (fk == FRAMEPOS_BT_EXTRINSICS && pair_cols[2*ip+1] < 0);
            if(kind == FRAMEPOS_NONE ? !(fk == FRAMEPOS_NONE || absent) : absent) consistent = false;
        }
    // (the splined models assemble from staged rows, not from Grams: no use for these tables)
    const bool uses_grams = D.lens_type != MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC;
    if(!consistent && uses_grams) { set_error("internal: the Gram positions of the frame part depend on the camera pair"); return false; }
    plan->obs_cols.assign(2*(size_t)Nobs, -1);
    for(int o = 0; o < Nobs; o++) for(int i = 0; i < 2; i++) plan->obs_cols[2*o + i] = pair_cols[2*plan->obs_pair[o] + i];
    return true;
}

// Observations of one frame are contiguous; the observations of one (intrinsics,extrinsics) pair are gathered in chunks
bool plan_board_grams(const DeviceProblem& D, const NormalDims& nd, const BoardObsMeta* meta, int Neblocks, BoardGramPlan* plan)
{
    *plan = BoardGramPlan();
    const int Nobs = D.Nobs_board;
    // the eliminated pose of an observation (its frame; with elim_extrinsics its camera, which may be the
    // reference: none then), and the one that stays in the camera block
    const bool elimx = nd.elim_extrinsics != 0;
    auto eblock_of = [&](const BoardObsMeta& m) -> int { return elimx ? m.icam_extrinsics : m.iframe; };
    // (what a Gram position means is common to the observations with the same camera-block columns AND the same
    //  columns present: the key of a "pair" carries whether there is an eliminated pose - a camera at the
    //  reference has none)
    auto spose_of  = [&](const BoardObsMeta& m) -> int { return 2*(elimx ? m.iframe : m.icam_extrinsics) + ((eblock_of(m) >= 0) ? 1 : 0); };
    auto same_pair = [&](int a, int b) -> bool { return meta[a].icam_intrinsics == meta[b].icam_intrinsics && spose_of(meta[a]) == spose_of(meta[b]); };
    std::vector<int>& frame_begin = plan->frame_obs_begin;
    frame_begin.assign(Neblocks+1, 0);
    for(int o=0;o<Nobs;o++) if(eblock_of(meta[o]) >= 0) frame_begin[eblock_of(meta[o])+1]++;
    for(int f=0;f<Neblocks;f++) frame_begin[f+1] += frame_begin[f];
    // sanity: contiguity
    for(int o=1;o<Nobs;o++)
        if(meta[o].iframe < meta[o-1].iframe) { set_error("board observations must be sorted by frame"); return false; }
    // (the observations of a frame are contiguous, those of a camera need not be: a list then)
    if(elimx)
    {
        std::vector<int> fill(frame_begin.begin(), frame_begin.end() - 1);
        plan->frame_obs.assign(Nobs, 0);
        for(int o=0;o<Nobs;o++) if(eblock_of(meta[o]) >= 0) plan->frame_obs[fill[eblock_of(meta[o])]++] = o;
    }

    std::vector<int>& order = plan->pair_obs;
    order.resize(Nobs);
    for(int o=0;o<Nobs;o++) order[o] = o;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b)
                     {
                         if(meta[a].icam_intrinsics != meta[b].icam_intrinsics) return meta[a].icam_intrinsics < meta[b].icam_intrinsics;
                         return spose_of(meta[a]) < spose_of(meta[b]);
                     });
    std::vector<int>& chunk_begin = plan->chunk_begin;
    for(int i=0;i<Nobs;)
    {
        int j = i;
        while(j < Nobs && j - i < REDUCE_CHUNK && same_pair(order[j], order[i])) j++;
        chunk_begin.push_back(i);
        i = j;
    }
    chunk_begin.push_back(Nobs);
    plan->Nchunks = (int)chunk_begin.size() - 1;
    // the (intrinsics, extrinsics) pairs, in the order of `order`
    std::vector<int> pair_rep;
    plan->obs_pair.assign(Nobs, 0);
    for(int k=0;k<Nobs;k++)
    {
        if(k == 0 || !same_pair(order[k], order[k-1])) pair_rep.push_back(order[k]);
        plan->obs_pair[order[k]] = (int)pair_rep.size() - 1;
    }
    plan->chunk_pair.assign(plan->Nchunks, 0);
    for(int c=0;c<plan->Nchunks;c++) plan->chunk_pair[c] = plan->obs_pair[order[chunk_begin[c]]];
    plan->Npairs = (int)pair_rep.size();

    const int nblk = tile_nblk(D.Ndist), npos = gram_stride(D.Ndist);
    std::vector<int>&    tab  = plan->pos_table;
    std::vector<PairOp>& ptab = plan->pair_table;
    tab.assign(npos, 0);
    ptab.assign(pair_rep.size()*npos, PairOp{PAIROP_NONE, 0});
    for(int pos = 0; pos < npos; pos++)
    {
        int i, j; bool diag;
        if(!gram_pos_to_entry(nblk, pos, &i, &j, &diag)) continue;
        tab[pos] = (int)(0x80000000u | (diag ? 0x10000u : 0u) | ((unsigned)i << 8) | (unsigned)j);
        for(size_t ip = 0; ip < pair_rep.size(); ip++)
        {
            const BoardObsMeta& m = meta[pair_rep[ip]];
            const TileColInfo ci = board_tile_col_info(D, m, i), cj = board_tile_col_info(D, m, j);
            PairOp op = { PAIROP_NONE, 0 };
            const bool fi = ci.kind == COL_FRAME, fj = cj.kind == COL_FRAME;
            const bool si = ci.kind == COL_S,     sj = cj.kind == COL_S;
            const bool xi = ci.kind == COL_X,     xj = cj.kind == COL_X;
            if(fi && fj)
                op = PairOp{ PAIROP_D | (diag ? 0 : PAIROP_MIRROR), ci.idx | (cj.idx << 16) };
            else if(fi)
            {
                // (frame, S) or (frame, x). In a diagonal block the mirrored
                // position carries the same product: it is taken there only
                if(!diag && sj)      op = PairOp{ PAIROP_BT, ci.idx | (state_to_SE(nd, cj.idx) << 16) };
                else if(!diag && xj) op = PairOp{ PAIROP_GF, ci.idx };
            }
            else if(fj)
            {
                if(si)      op = PairOp{ PAIROP_BT, cj.idx | (state_to_SE(nd, ci.idx) << 16) };
                else if(xi) op = PairOp{ PAIROP_GF, cj.idx };
            }
            else if((si || xi) && (sj || xj) && !(diag && xi && sj))
            {
                if(xi && xj)   op = PairOp{ PAIROP_NORM, 0 };
                else if(xj)    op = PairOp{ PAIROP_G, ci.idx };
                else if(xi)    op = PairOp{ PAIROP_G, cj.idx };
                else           op = PairOp{ PAIROP_A | (diag ? 0 : PAIROP_MIRROR),
                                            state_to_SE(nd, ci.idx) | (state_to_SE(nd, cj.idx) << 16) };
            }
            ptab[ip*npos + pos] = op;
            const int k = op.op & 0xff;
            if(k == PAIROP_D || k == PAIROP_BT || k == PAIROP_GF) tab[pos] |= 0x20000;
        }
    }
    if(!plan_frame_part(D, nd, meta, pair_rep, plan)) return false;

    // The fixed-order reduction of the camera-block part (solver_kernels.hpp):
    // for every destination - entry of A, of g (S part), |x|^2 - the (pair,
    // position) sources that add to it, in (pair, position) order
    // (the splined models have no Grams: nothing is reduced this way)
    const bool with_grams = D.lens_type != MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC;
    const int Npairs = with_grams ? (int)pair_rep.size() : 0;
    if(with_grams && npos > 1024) { set_error("internal error: %d Gram positions per observation", npos); return false; }
    plan->pair_chunk_begin.assign(Npairs + 1, 0);
    for(int c=0;c<plan->Nchunks && Npairs > 0;c++) plan->pair_chunk_begin[plan->chunk_pair[c] + 1]++;
    for(int ip=0;ip<Npairs;ip++) plan->pair_chunk_begin[ip+1] += plan->pair_chunk_begin[ip];
    const int nA = nd.Nc*nd.Nc;
    DestSources src;
    // |x|^2 is always a destination when there are rows outside the Grams (their partials are added there)
    if(Npairs > 0) src[nA + nd.Nc];
    for(int ip = 0; ip < Npairs; ip++)
        for(int pos = 0; pos < npos; pos++)
        {
            const PairOp op = ptab[(size_t)ip*npos + pos];
            const int k = op.op & 0xff, code = (ip << 10) | pos;
            if(k == PAIROP_NORM) src[nA + nd.Nc].push_back(code);
            else if(k == PAIROP_G)
            {
                const int sc = state_to_SE(nd, op.aux);     // a camera-block variable: S index >= 0
                if(sc >= 0) src[nA + sc].push_back(code);
            }
            else if(k == PAIROP_A)
            {
                const int a = op.aux & 0xffff, b = op.aux >> 16;
                src[a*nd.Nc + b].push_back(code);
                if(op.op & PAIROP_MIRROR) src[b*nd.Nc + a].push_back(code);
            }
        }
    plan->dest = make_dest_lists(src);
    return true;
}

// The fixed-order plan for the rows outside the Grams that share destinations: discrete points, triangulated
// pairs (GenPlan, solver_kernels.hpp). From the CSR structure itself, which does not change between evaluations
GenRowsPlan plan_gen_rows(const NormalDims& nd, int r0, int r1, const int32_t* Jp, const int32_t* Ji)
{
    const GenRowsPlan none;
    GenRowsPlan G;
    if(r1 <= r0) return none;
    const int32_t p0 = Jp[0];
    struct RowInfo { int group, eblk, epos; };
    std::vector<RowInfo> info((size_t)(r1 - r0));
    // a row's signature [k | spos.. | scol..] -> its group, the groups numbered as they first appear. (Round 6: the
    // signature on the stack and a hash in front of the comparison; three vectors and an ordered map of vectors a row
    // were 10 ms of BASELINE configuration 4's 67 000 rows - as long as its five dog-leg steps and their launches together)
    std::unordered_map<uint64_t, std::vector<int>> groups;
    std::vector<std::vector<int>> group_sig;
    bool any_eblock = false;
    for(int r = r0; r < r1; r++)
    {
        const int a = Jp[r - r0] - p0, b = Jp[r - r0 + 1] - p0;
        int sig[2*GEN_KMAX + 1], scol[GEN_KMAX];
        int k = 0;
        int eblk = -1, epos = -1, ecount = 0;
        for(int p = a; p < b; p++)
        {
            const int c = Ji[p];
            if(c < 0 || c >= nd.Nstate) return none;                 // (flagged at run time by the row-by-row path)
            const int se = state_to_SE(nd, c);
            if(se >= 0)
            {
                if(k >= GEN_KMAX) return none;
                sig[1 + k] = p - a; scol[k] = se; k++;
            }
            else
            {
                const int e = -se - 1;
                const int blk = (e < 6*nd.Nfb) ? e/6 : nd.Nfb + (e - 6*nd.Nfb)/3;
                const int e0  = (blk < nd.Nfb) ? 6*blk : 6*nd.Nfb + 3*(blk - nd.Nfb);
                const int de  = (blk < nd.Nfb) ? 6 : 3;
                // the block's columns must be all there, side by side, in order
                if(ecount == 0) { if(e != e0) return none; eblk = blk; epos = p - a; }
                else if(blk != eblk || e != e0 + ecount || p - a != epos + ecount) return none;
                ecount++;
                if(ecount > de) return none;
            }
        }
        if(eblk >= 0 && ecount != ((eblk < nd.Nfb) ? 6 : 3)) return none;
        any_eblock = any_eblock || eblk >= 0;
        if(k > G.kmax) G.kmax = k;
        sig[0] = k;
        for(int i = 0; i < k; i++) sig[1 + k + i] = scol[i];
        const int nsig = 2*k + 1;
        uint64_t h = 1469598103934665603ull;
        for(int i = 0; i < nsig; i++) { h ^= (uint64_t)(uint32_t)sig[i]; h *= 1099511628211ull; }
        std::vector<int>& cand = groups[h];
        int g = -1;
        for(int gc : cand)
            if((int)group_sig[gc].size() == nsig && !memcmp(group_sig[gc].data(), sig, nsig*sizeof(int))) { g = gc; break; }
        if(g < 0) { g = (int)group_sig.size(); cand.push_back(g); group_sig.emplace_back(sig, sig + nsig); }
        info[r - r0] = RowInfo{ g, eblk, epos };
    }
    const int Ngroups = (int)group_sig.size();
    G.stride = (G.kmax*(G.kmax+1))/2 + G.kmax + 1;
    if(G.stride > 1023 || Ngroups >= (1 << 20)) return none;
    // (gen_eblock keeps a block's rows of Bt in LDS: 6 Nc doubles, within the 64 KB a launch gets without asking)
    if(any_eblock && ((size_t)6*nd.Nc + 42)*sizeof(double) > 64*1024) return none;

    // rows by (group, row); chunks
    // (by counting: the groups are few)
    G.rows.resize((size_t)(r1 - r0));
    {
        std::vector<int> at(Ngroups + 1, 0);
        for(const RowInfo& ri : info) at[ri.group + 1]++;
        for(int g = 0; g < Ngroups; g++) at[g + 1] += at[g];
        for(int i = 0; i < r1 - r0; i++) G.rows[at[info[i].group]++] = r0 + i;
    }
    G.group_chunk_begin.assign(Ngroups + 1, 0);
    for(size_t i = 0; i < G.rows.size();)
    {
        const int g = info[G.rows[i] - r0].group;
        size_t j = i;
        while(j < G.rows.size() && j - i < GEN_CHUNK && info[G.rows[j] - r0].group == g) j++;
        G.chunk_begin.push_back((int)i); G.chunk_group.push_back(g);
        G.group_chunk_begin[g + 1]++;
        i = j;
    }
    G.chunk_begin.push_back((int)G.rows.size());
    for(int g = 0; g < Ngroups; g++) G.group_chunk_begin[g+1] += G.group_chunk_begin[g];
    G.group_k.resize(Ngroups); G.group_off.resize(Ngroups);
    for(int g = 0; g < Ngroups; g++)
    {
        const std::vector<int>& sig = group_sig[g];
        const int k = sig[0];
        G.group_k[g] = k; G.group_off[g] = (int)G.spos.size();
        G.spos.insert(G.spos.end(), sig.begin() + 1, sig.begin() + 1 + k);
        G.scol.insert(G.scol.end(), sig.begin() + 1 + k, sig.end());
    }
    // destinations: entries of A (both orientations, as the row-by-row path adds them), of g (S part), |x|^2
    const int nA = nd.Nc*nd.Nc;
    DestSources src;
    for(int g = 0; g < Ngroups; g++)
    {
        const int k = G.group_k[g];
        const int* sc = G.scol.data() + G.group_off[g];
        int pos = 0;
        for(int p = 0; p < k; p++)
            for(int q = p; q < k; q++, pos++)
            {
                const int code = (g << 10) | pos;
                src[sc[p]*nd.Nc + sc[q]].push_back(code);
                if(q != p) src[sc[q]*nd.Nc + sc[p]].push_back(code);
            }
        for(int p = 0; p < k; p++, pos++) src[nA + sc[p]].push_back((g << 10) | pos);
        src[nA + nd.Nc].push_back((g << 10) | pos);
    }
    G.dest = make_dest_lists(src);
    // the eliminated blocks: their rows, in row order
    std::map<int, std::vector<int>> by_block;
    for(int r = r0; r < r1; r++)
        if(info[r - r0].eblk >= 0) by_block[info[r - r0].eblk].push_back(r);
    G.eb_begin.push_back(0);
    for(auto& kv : by_block)
    {
        G.eb_block.push_back(kv.first);
        for(int r : kv.second) { G.eb_rows.push_back(r); G.eb_group.push_back(info[r - r0].group); G.eb_epos.push_back(info[r - r0].epos); }
        G.eb_begin.push_back((int)G.eb_rows.size());
    }
    G.Nrows = r1 - r0; G.Nchunks = (int)G.chunk_group.size(); G.Ngroups = Ngroups;
    return G;
}

} // namespace mrcal_amd

// dev / tests (no declaration in include/: not part of the interface), as mrcal_amd_debug_lchol_plan. Need no GPU.
// Both write [count | entries] list after list into out[capacity] and return the ints that takes (more than capacity:
// nothing was written)
static int flatten(const std::vector<const std::vector<int>*>& lists, const std::vector<int>& head, int* out, int capacity)
{
    size_t n = head.size();
    for(const std::vector<int>* v : lists) n += 1 + v->size();
    if(n > (size_t)capacity) return (int)n;
    out = std::copy(head.begin(), head.end(), out);
    for(const std::vector<int>* v : lists) { *out++ = (int)v->size(); out = std::copy(v->begin(), v->end(), out); }
    return (int)n;
}
// plan_gen_rows() of rows [0, Nrows) under the frames partition of a state [Nshared intrinsics + extrinsics | Nfb frames |
// Npb points | Nwarp]. out: Nrows, Nchunks, Ngroups, stride, kmax, Ndest, Neblocks, then GenPlan's lists in its field order
extern "C" int mrcal_amd_debug_plan_gen_rows(int Nshared, int Nfb, int Npb, int Nwarp, int Nrows,
                                             const int32_t* rowptr, const int32_t* colidx, int* out, int capacity)
{
    using namespace mrcal_amd;
    NormalDims nd;
    memset(&nd, 0, sizeof(nd));
    nd.Nfb = Nfb; nd.Npb = Npb; nd.NEb = Nfb + Npb; nd.NE = 6*Nfb + 3*Npb;
    nd.Nwarp = Nwarp; nd.Nc = Nshared + Nwarp;
    nd.i_state_warp = Nshared + nd.NE; nd.Nstate = nd.i_state_warp + Nwarp;
    normal_dims_set_partition(nd, Nshared);
    const GenRowsPlan G = plan_gen_rows(nd, 0, Nrows, rowptr, colidx);
    return flatten({ &G.rows, &G.chunk_begin, &G.chunk_group, &G.group_k, &G.group_off, &G.spos, &G.scol,
                     &G.dest.id, &G.dest.begin, &G.dest.src, &G.group_chunk_begin,
                     &G.eb_block, &G.eb_begin, &G.eb_rows, &G.eb_group, &G.eb_epos },
                   { G.Nrows, G.Nchunks, G.Ngroups, G.stride, G.kmax, (int)G.dest.id.size(), (int)G.eb_block.size() }, out, capacity);
}
// make_dest_lists() of the sources (dest[i], code[i]), i = 0 .. n-1, in that order. out: dest_id, dest_begin, dest_src
extern "C" int mrcal_amd_debug_dest_lists(int n, const int* dest, const int* code, int* out, int capacity)
{
    mrcal_amd::DestSources src;
    for(int i = 0; i < n; i++) src[dest[i]].push_back(code[i]);
    const mrcal_amd::DestLists d = mrcal_amd::make_dest_lists(src);
    return flatten({ &d.id, &d.begin, &d.src }, {}, out, capacity);
}
