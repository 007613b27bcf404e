O=gpurun_out/r05; mkdir -p $O; export TMPDIR=/tmp
R=$PWD/tools/ab/lib_r04.so
tools/abn.sh 4 "--steps 20 --warmup 5" "PF_LIB=$R" "PF_X=1" > $O/ab12_driver.txt 2>&1; cat $O/ab12_driver.txt
python bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/r05_bench_driver.json 2> $O/r05_bench_driver.err; echo "driver rc $?"
python bench.py --full > $O/r05_bench_default.json 2> $O/r05_bench_default.err; echo "default rc $?"
python bench.py --int16 --no-cpu > $O/r05_bench_int16.json 2>/dev/null
PF_DIST_BACKEND=gloo python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29517 bench.py --full --gpus 2 --steps 20 --warmup 5 --no-cpu > $O/r05_default_2ranks_gloo_one_gpu.json 2> $O/r05_2ranks.err; echo "2 ranks rc $?"
PF_DIST_BACKEND=gloo python -m torch.distributed.run --nnodes=1 --nproc-per-node 4 --master-addr 127.0.0.1 --master-port 29518 bench.py --gpus 4 --steps 20 --warmup 5 --no-cpu --shard strong > $O/r05_strong_4ranks_gloo_one_gpu.json 2> $O/r05_4ranks.err; echo "4 ranks rc $?"
python - <<'PY'
import json
for f in ("r05_bench_driver","r05_bench_default","r05_bench_int16","r05_default_2ranks_gloo_one_gpu","r05_strong_4ranks_gloo_one_gpu"):
    try:
        j=json.load(open("gpurun_out/r05/%s.json"%f)); r=j["roofline"]
        print(f, j["value"], j["ms_per_step"], j["scaling"], {k:r.get(k) for k in ("frac","frac_full_canvas","frac_delivered","avg_launch_us","traffic","alg_bytes_run_per_launch","window")}, "pmc current:", (r.get("pmc_build") or {}).get("current"))
        for k in ("int16","full_render_no_cull","cpu_baseline","cpu_baseline_allcores","host_feed"):
            if k in j: print("   ", k, json.dumps(j[k])[:260])
    except Exception as e: print(f, "ERR", e)
PY
