#!/bin/bash
OUT=$GRAFT_REPO_ROOT/gpurun_out/${1:-r05blk}; mkdir -p $OUT; cd $GRAFT_REPO_ROOT
timeout 1500 python -m pytest tests/test_taxim_gpu.py tests/test_sensor_gpu.py tests/test_edge_cases_gpu.py tests/test_sensor_configs_gpu.py tests/test_height_map_source.py tests/test_mesh_depth.py -x -q -m gpu 2>&1 | tail -8 | tee $OUT/test.log
bash scripts/ab_r05.sh ${1:-r05blk} "noblk _" 3
for tag in noblk _; do t=$tag; [ "$tag" = "_" ] && t=""
TACEX_LIB_TAG=$t TACEX_LIB_FROZEN=1 timeout 600 python bench.py --full --no-cpu-baseline --steps 10 --sweep-keys c3_dense,c2,c5_optical,ref_scene,shard512 --details-out $OUT/d2.json > /dev/null 2>$OUT/err2.log; echo "[$tag]"; python scripts/print_sweep.py $OUT/d2.json | tee -a $OUT/sweep.log
done
