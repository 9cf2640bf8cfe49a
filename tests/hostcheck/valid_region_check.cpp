// Drives csrc/region_outline.cpp as a stand-alone program (built with ASan + UBSan by
// tests/hostbuild.py for tests/test_valid_region_host.py). Reads masks from the file named on the command line, one a line:
//   w h c c c ...      (w*h cells, 0 or 1, row-major)
// and prints for each:  nvertices area2 x y x y ...   through the C entry point, with a capacity one short of what is
// needed first, to see that nothing is written beyond it.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../mrcal_amd/csrc/region_outline.hpp"

int main(int argc, char** argv)
{
    if(argc != 2) { fprintf(stderr, "usage: %s masks.txt\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if(!f) { perror(argv[1]); return 2; }
    int w, h;
    while(fscanf(f, "%d %d", &w, &h) == 2)
    {
        if(w <= 0 || h <= 0 || (long)w*h > 1000000) { fprintf(stderr, "bad size\n"); return 2; }
        std::vector<uint8_t> mask((size_t)w*h);
        for(size_t i = 0; i < mask.size(); i++)
        {
            int c;
            if(fscanf(f, "%d", &c) != 1) { fprintf(stderr, "short mask\n"); return 2; }
            mask[i] = (uint8_t)c;
        }
        int64_t area2 = -1;
        const int n = mrcal_amd_region_outline(mask.data(), w, h, NULL, 0, &area2);
        if(n < 0) { fprintf(stderr, "refused\n"); return 1; }
        // exactly n entries: ASan sees a write past them; and one short, where the last must stay untouched
        std::vector<int32_t> v((size_t)2*n), shorter((size_t)2*(n > 0 ? n - 1 : 0));
        int64_t area2_again = -1;
        if(mrcal_amd_region_outline(mask.data(), w, h, v.data(), n, &area2_again) != n || area2_again != area2) return 1;
        if(n > 0 && mrcal_amd_region_outline(mask.data(), w, h, shorter.data(), n - 1, NULL) != n) return 1;
        for(size_t i = 0; i < shorter.size(); i++) if(shorter[i] != v[i]) return 1;
        printf("%d %lld", n, (long long)area2);
        for(int i = 0; i < n; i++) printf(" %d %d", v[2*i], v[2*i + 1]);
        printf("\n");
    }
    fclose(f);
    // the refusals
    uint8_t one = 1;
    if(mrcal_amd_region_outline(NULL, 1, 1, NULL, 0, NULL) != -1 || mrcal_amd_region_outline(&one, 0, 1, NULL, 0, NULL) != -1 ||
       mrcal_amd_region_outline(&one, 1, 1, NULL, 1, NULL) != -1)
        return 1;
    return 0;
}
