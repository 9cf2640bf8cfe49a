# -DLCH_TS: the launch-per-panel Cholesky's diagonal and tile workgroups (BASELINE configuration 2: a 1206-variable camera block)
MRCAL_AMD_LIB=mrcal_amd/libmrcal_amd_dev.so timeout 300 python tools/probe_config2.py 2>&1 | python tools/cycle_stamps.py
