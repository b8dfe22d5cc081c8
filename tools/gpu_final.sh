#!/bin/bash
# end-of-round evidence (one session, one box): tests, smoke, kbench, bench (plain + torchrun), rocprof kernel stats of the bench loop
# and of the config-3 step, PMC traffic + SQ counters (config 2 and 5), config 5 incl. objective legs, batch sweep, host overhead.
# Everything lands in $OUT_DIR/; copy what is to be judged into profiles/.
set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT_DIR=${SGR_OUT_DIR:-$ROOT/bench_out}
cd "$ROOT"
mkdir -p $OUT_DIR
export TMPDIR=/tmp
LIB=inverserenderingofindoorscene_amd/libsgrender.so
echo "== pytest gpu"; t0=$SECONDS; timeout 1500 python -m pytest tests -q -m gpu --durations=6 -s > $OUT_DIR/pytest_gpu.txt 2>&1; echo "pytest wall $((SECONDS-t0)) s"; tail -10 $OUT_DIR/pytest_gpu.txt | cut -c1-200
echo "== smoke"; timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2 | tee $OUT_DIR/smoke.txt | cut -c1-600
echo "== kbench"; timeout 300 ./tools/kbench $LIB 16 20 > $OUT_DIR/kbench.txt 2>&1; cat $OUT_DIR/kbench.txt
# bench.py writes the ONE JSON line to stdout and everything else (RCCL's banner included) to stderr: keep the two apart
echo "== bench"; t0=$SECONDS; timeout 900 python bench.py --full > $OUT_DIR/bench.txt 2> $OUT_DIR/bench.err; echo "bench wall $((SECONDS-t0)) s, stdout lines: $(wc -l < $OUT_DIR/bench.txt), line bytes: $(wc -c < $OUT_DIR/bench.txt)" | tee $OUT_DIR/bench_time.txt; tail -1 $OUT_DIR/bench.txt | cut -c1-3200; cp bench_detail.json $OUT_DIR/bench_detail.json
echo "== bench with the driver's flags, --full"; t0=$SECONDS; timeout 600 python bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT_DIR/bench_warmup5.txt 2> $OUT_DIR/bench_warmup5.err; echo "wall $((SECONDS-t0)) s"; tail -1 $OUT_DIR/bench_warmup5.txt | cut -c1-900; cp bench_detail.json $OUT_DIR/bench_warmup5_detail.json
echo "== bench --gpus 2 / 4 / 8 WITHOUT torchrun over gloo on this one GPU (rehearsal of the driver's N > 1 launches: flagged config.rehearsal, no measurement)"; for n in 2 4 8; do SGR_BENCH_BACKEND=gloo SGR_BENCH_DETAIL=$OUT_DIR/rehearsal_n${n}_detail.json timeout 900 python bench.py --full --gpus $n --steps 5 --warmup 3 --reps 3 > $OUT_DIR/rehearsal_n$n.json 2> $OUT_DIR/rehearsal_n$n.err; echo "N=$n rc=$? $(cut -c1-160 $OUT_DIR/rehearsal_n$n.json)"; done
echo "== bench torchrun world=1 (RCCL init / barrier / all-reduce path)"; timeout 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29531 bench.py --full --gpus 1 --no-cpu-baseline --layer-only > $OUT_DIR/bench_torchrun1.txt 2> $OUT_DIR/bench_torchrun1.err; tail -1 $OUT_DIR/bench_torchrun1.txt | cut -c1-500
echo "== host overhead"; timeout 300 python tools/host_overhead.py 2>&1 | tail -10 | tee $OUT_DIR/host_overhead.txt
echo "== rocprof bench loop"; cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT_DIR/prof -- python $ROOT/bench.py --full --steps 20 --warmup 20 --reps 2 --no-cpu-baseline --no-config5 > $OUT_DIR/rocprof.txt 2>&1; cd $ROOT
for f in $(find $OUT_DIR/prof -name "*kernel_stats.csv" | head -1); do cp $f $OUT_DIR/kernel_stats.csv; head -12 $f | cut -c1-200; done
find $OUT_DIR/prof -name "*kernel_trace.csv" -size +1M -delete
echo "== rocprof config-3 step (examples/train_light_synthetic.py)"; cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT_DIR/prof3 -- python $ROOT/examples/train_light_synthetic.py --batch 16 --steps 43 > $OUT_DIR/rocprof3.txt 2>&1; cd $ROOT
tail -1 $OUT_DIR/rocprof3.txt
for f in $(find $OUT_DIR/prof3 -name "*kernel_stats.csv" | head -1); do cp $f $OUT_DIR/kernel_stats_config3.csv; python tools/config3_breakdown.py $f 43 | tee $OUT_DIR/config3_breakdown.txt; done
find $OUT_DIR/prof3 -name "*kernel_trace.csv" -size +1M -delete
echo "== pmc traffic config 2"; bash tools/pmc_traffic.sh config2_batch16_env | grep -E "fwd_pk|sg_bwd_pk"
echo "== pmc sq config 2"; bash tools/pmc_sq.sh config2_batch16_env | grep -E "fwd_pk|sg_bwd_pk"
# round 4: the kernels of the real trainLight step -- the fused objective (premap 1) and with the decoder heads as prologue (premap 3)
echo "== pmc traffic config 2, objective"; bash tools/pmc_traffic.sh config2_batch16_objective --pmc-workload objective | grep -E "fwd_pk|sg_bwd_recon"
echo "== pmc sq config 2, objective"; bash tools/pmc_sq.sh config2_batch16_objective --pmc-workload objective | grep -E "fwd_pk|sg_bwd_recon"
echo "== pmc traffic config 2, objective + heads"; bash tools/pmc_traffic.sh config2_batch16_objective_heads --pmc-workload objective_heads | grep -E "fwd_pk|sg_bwd_recon"
echo "== pmc sq config 2, objective + heads"; bash tools/pmc_sq.sh config2_batch16_objective_heads --pmc-workload objective_heads | grep -E "fwd_pk|sg_bwd_recon"
echo "== pmc traffic config 5"; bash tools/pmc_traffic.sh config5_batch4_env --config 5 | grep -E "fwd_pk|sg_bwd_pk"
echo "== pmc sq config 5"; bash tools/pmc_sq.sh config5_batch4_env --config 5 | grep -E "fwd_pk|sg_bwd_pk"
echo "== pmc traffic config 5, objective"; bash tools/pmc_traffic.sh config5_batch4_objective --config 5 --pmc-workload objective | grep -E "fwd_pk|sg_bwd_recon"
echo "== pmc sq config 5, objective"; bash tools/pmc_sq.sh config5_batch4_objective --config 5 --pmc-workload objective | grep -E "fwd_pk|sg_bwd_recon"
echo "== config 5"; timeout 900 python bench.py --full --config 5 --no-cpu-baseline > $OUT_DIR/bench_config5.txt 2> $OUT_DIR/bench_config5.err; tail -1 $OUT_DIR/bench_config5.txt | cut -c1-1800
# the counter records are fresh now: the line of record carries them un-stale (config 5's leg included)
echo "== bench with the fresh counter records (driver-style flags)"; cp $OUT_DIR/traffic.json profiles/traffic.json; cp $OUT_DIR/sq.json profiles/sq.json; timeout 900 python bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT_DIR/bench_fresh_records.txt 2> $OUT_DIR/bench_fresh_records.err; tail -1 $OUT_DIR/bench_fresh_records.txt | cut -c1-3200; cp bench_detail.json $OUT_DIR/bench_fresh_records_detail.json
echo "== FETCH_SIZE calibration on known byte counts (tools/fetch_calib)"; timeout 300 ./tools/fetch_calib 10 | tee $OUT_DIR/fetch_calib_timing.txt
(cd /tmp && timeout 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT_DIR/calib_fetch -- $ROOT/tools/fetch_calib 1 > /dev/null 2>&1; timeout 300 rocprofv3 --kernel-trace --pmc TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum --output-format csv -d $OUT_DIR/calib_rdreq -- $ROOT/tools/fetch_calib 1 > /dev/null 2>&1)
python tools/fetch_calib_report.py $OUT_DIR | tee $OUT_DIR/fetch_calib_counters.txt
echo "== wavetrace (schedule + shader clock under load)"; if [ -f inverserenderingofindoorscene_amd/variants/libsgrender_trace.so ]; then timeout 300 ./tools/wavetrace inverserenderingofindoorscene_amd/variants/libsgrender_trace.so 16 > /tmp/trace.txt 2>/dev/null; python tools/wavetrace_report.py /tmp/trace.txt > $OUT_DIR/wavetrace_report.txt 2>&1; grep -E "^[a-z_0-9]+:|shader clock" $OUT_DIR/wavetrace_report.txt | cut -c1-200; fi
echo "== batch sweep"; for b in 5 8 16 32 64; do st=100; wu=300; if [ $b -ge 32 ]; then st=40; wu=80; fi; timeout 300 python bench.py --full --batch $b --steps $st --warmup $wu --no-cpu-baseline --layer-only --graph-leg 2>/dev/null | tail -1 | python -c "
import json,sys
d=json.loads(sys.stdin.read()); c=d['config']; g=c.get('ms_with_loss_graph'); print('batch $b', d['value'], 'Mpix/s', d['ms_per_step'], 'ms/step  fwd', c['fwd_us'], 'us  bwd', c['bwd_us'], 'us  with loss', c['Mpix_with_loss'], 'Mpix/s  with loss, replayed from a HIP graph', None if g is None else round($b * 240 * 320 / (g * 1e-3) / 1e6, 1))"; done | tee $OUT_DIR/bench_batch_sweep.txt
echo "== trainlight example (fused objective + HIP heads | unfused + torch heads)"
timeout 300 python examples/train_light_synthetic.py --batch 16 --steps 23 2>&1 | tail -1 | tee $OUT_DIR/trainlight_fused.txt
timeout 300 python examples/train_light_synthetic.py --batch 16 --steps 23 --unfused --torch-heads 2>&1 | tail -1 | tee $OUT_DIR/trainlight_unfused.txt
