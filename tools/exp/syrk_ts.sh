# -DSYRK_TS: the sparse SYRK's scan / blocks, the blocks that count per strip; then configuration 2's kernel table
MRCAL_AMD_LIB=mrcal_amd/libmrcal_amd_dev.so timeout 300 python tools/probe_config2.py 2>&1 | python tools/cycle_stamps.py
bash tools/exp/c2_quick.sh 2>&1 | grep -v "^ts \|^W2026"
