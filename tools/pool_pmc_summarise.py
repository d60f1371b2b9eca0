#!/usr/bin/env python3
"""Summarise a profile of the pool search kernel (search_f64_kernel_pool): the --kernel-trace --stats table of one run and the
--pmc passes of others (each pass a run of its own, no tracing beside --pmc).
usage: pool_pmc_summarise.py <dir with stats/ and pmc*/> <batch>
The directory is filled by (ARGS: --no-cpu-baseline --no-configs, plus --batch 65536 --in-flight 1 for the large batch)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/stats -- python3 bench.py --gpus 1 --steps 200 --warmup 20 ARGS
    rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY \
              --output-format csv -d DIR/pmc1 -- python3 bench.py --gpus 1 --steps 20 --warmup 3 ARGS
    ... --pmc GRBM_GUI_ACTIVE SQ_WAIT_INST_ANY -d DIR/pmc2 ...;  ... --pmc SQ_INSTS_LDS SQ_INSTS_SMEM SQ_INSTS_VMEM -d DIR/pmc3 ...
Prints one JSON record: the kernel's share of the GPU time, mean duration, and per launch / per scenario the VALU, SALU, LDS
instruction counts and VALU-busy.  Under --pmc the dispatches are serialised, so the counters describe the kernel running alone."""
import csv, glob, json, os, sys
from collections import defaultdict

KEY = 'search_f64_kernel_pool'
SIMDS = 1024            # MI355X: 256 compute units x 4 SIMDs
XCDS = 8                # GRBM_GUI_ACTIVE is summed over the XCDs
QUAD = 4.0              # SQ_* cycle counters count quad-cycles


def main(root, B):
    out = {'kernel': KEY, 'batch': B}
    for f in glob.glob(os.path.join(root, 'stats', '**', '*kernel_stats.csv'), recursive=True):
        with open(f) as fh:
            rows = list(csv.DictReader(fh))
        tot = sum(float(r['TotalDurationNs']) for r in rows)
        out['stats_top'] = [{'name': r['Name'][:100], 'calls': int(r['Calls']), 'avg_ns': float(r['AverageNs']),
                             'share_of_gpu_time': float(r['TotalDurationNs']) / tot} for r in rows[:8]]
        for r in rows:
            if KEY in r['Name']:
                out['pool_kernel'] = {'calls': int(r['Calls']), 'avg_ns': float(r['AverageNs']), 'min_ns': float(r['MinNs']),
                                      'max_ns': float(r['MaxNs']), 'share_of_gpu_time': float(r['TotalDurationNs']) / tot}
    c, info = {}, {}
    for d in sorted(glob.glob(os.path.join(root, 'pmc*'))):
        per, dur = defaultdict(float), {}
        for f in glob.glob(os.path.join(d, '**', '*counter_collection.csv'), recursive=True):
            with open(f) as fh:
                recs = list(csv.DictReader(fh))
            for r in recs:
                if KEY in r['Kernel_Name']:
                    per[(r['Counter_Name'], int(r['Dispatch_Id']))] += float(r['Counter_Value'])
                    if r.get('End_Timestamp') and r.get('Start_Timestamp'):
                        dur[int(r['Dispatch_Id'])] = float(r['End_Timestamp']) - float(r['Start_Timestamp'])
                    for k in ('VGPR_Count', 'Accum_VGPR_Count', 'SGPR_Count', 'LDS_Block_Size', 'Scratch_Size'):
                        if r.get(k):
                            info[k] = r[k]
        by = defaultdict(list)
        for (cn, did), v in sorted(per.items(), key=lambda kv: kv[0][1]):
            by[cn].append(v)
        for cn, v in by.items():
            v = v[len(v) // 4:]                      # skip warm-up launches
            c[cn] = sum(v) / len(v)
            out.setdefault('launches_counted', {})[cn] = len(v)
        if dur and 'SQ_INSTS_VALU' in by:
            v = [dur[k] for k in sorted(dur)]
            v = v[len(v) // 4:]
            c['dur_ns_in_valu_pass'] = sum(v) / len(v)
    out['counters_mean_per_launch'] = c
    out['kernel_info'] = info
    d = {}
    if 'SQ_INSTS_VALU' in c:
        d['waves_per_launch'] = c.get('SQ_WAVES')
        for k in ('VALU', 'SALU', 'LDS', 'SMEM', 'VMEM'):
            if f'SQ_INSTS_{k}' in c:
                d[f'{k.lower()}_instructions_per_scenario'] = c[f'SQ_INSTS_{k}'] / B
        d['busy_cycles_per_valu_instruction'] = QUAD * c['SQ_ACTIVE_INST_VALU'] / c['SQ_INSTS_VALU']
        if 'dur_ns_in_valu_pass' in c:
            clk = c['GRBM_GUI_ACTIVE'] / XCDS / c['dur_ns_in_valu_pass'] if 'GRBM_GUI_ACTIVE' in c else 2.4
            simd_cycles = SIMDS * c['dur_ns_in_valu_pass'] * clk
            d['clock_GHz_assumed'] = clk
            d['simd_valu_busy_fraction'] = QUAD * c['SQ_ACTIVE_INST_VALU'] / simd_cycles
            d['mean_waves_resident_per_simd'] = QUAD * c['SQ_WAVE_CYCLES'] / simd_cycles
        if 'SQ_WAVE_CYCLES' in c:
            d['valu_active_share_of_wave_cycles'] = c['SQ_ACTIVE_INST_VALU'] / c['SQ_WAVE_CYCLES']
            d['any_active_share_of_wave_cycles'] = c.get('SQ_ACTIVE_INST_ANY', 0.0) / c['SQ_WAVE_CYCLES']
    out['derived'] = d
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == '__main__':
    main(sys.argv[1], int(sys.argv[2]))
