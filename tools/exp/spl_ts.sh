# -DSPL_TS / -DSPLG_TS: the splined assembly's phases per workgroup and the workgroups' places in time (wall0, wall1), the gather's laps
MRCAL_AMD_LIB=mrcal_amd/libmrcal_amd_dev.so timeout 300 python tools/probe_config2.py 2>&1 | python tools/cycle_stamps.py
