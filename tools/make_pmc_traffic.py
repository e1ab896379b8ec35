"""profiles/r01_pmc_hbm_traffic.json from two rocprofv3 counter-collection CSVs (one --pmc FETCH_SIZE pass, one --pmc
WRITE_SIZE pass -- never combined with each other or with tracing domains other than --kernel-trace):

    python tools/make_pmc_traffic.py <fetch_counter_collection.csv> <write_counter_collection.csv> <out.json>

Units / corrections as MI355X_MICROARCH.md prescribes: both counters are in KB; FETCH_SIZE is doubled on gfx950 (128-byte read
requests are tallied at 64 B for wide coalesced reads)."""
import collections
import csv
import json
import re
import sys


def per_kernel(path, counter):
    tot, n = collections.defaultdict(float), collections.Counter()
    for r in csv.DictReader(open(path)):
        if r['Counter_Name'] != counter:
            continue
        k = re.sub(r'^void ', '', r['Kernel_Name']).replace('(anonymous namespace)::', '')
        k = k.split('(')[0] if '<' not in k.split('(')[0] else k[:k.index('>') + 1]
        tot[k] += float(r['Counter_Value'])
        n[k] += 1
    return tot, n


def main():
    fetch, nf = per_kernel(sys.argv[1], 'FETCH_SIZE')
    write, nw = per_kernel(sys.argv[2], 'WRITE_SIZE')
    kernels = []
    for k in sorted(fetch, key=lambda k: -(2 * fetch[k] + write.get(k, 0.0))):
        if nf[k] == 0 or nw.get(k, 0) == 0:
            continue
        f, w = fetch[k] / nf[k], write[k] / nw[k]
        kernels.append({'kernel': k, 'launches': nf[k], 'FETCH_SIZE_KB_per_launch': round(f, 1), 'WRITE_SIZE_KB_per_launch': round(w, 1),
                        'hbm_bytes_per_launch_corrected': int((2 * f + w) * 1024)})
    # the 3x3 forward + data-gradient family: Winograd kernels (fp32), or the direct KIND = 0 kernel + the persistent bf16 kernel
    fam = [k for k in kernels if k['kernel'].startswith(('wino_conv_kernel', 'wino_ring_kernel'))] or \
          [k for k in kernels if re.match(r'conv_mfma_kernel<\d+, \d+, \d+, \d+, 0,', k['kernel']) or
           k['kernel'].startswith(('conv_gemm16p_kernel', 'conv_ring16_kernel'))]
    n = sum(k['launches'] for k in fam)
    out = {
        'source': 'rocprofv3 --kernel-trace --pmc FETCH_SIZE  /  --pmc WRITE_SIZE (two separate passes) -- python bench.py --full --steps 3 --warmup 2 --no-cpu-baseline',
        'units': 'FETCH_SIZE / WRITE_SIZE are reported in KB; FETCH_SIZE is doubled (gfx950 tallies 128-B read requests at 64 B for '
                 'wide coalesced reads, MI355X_MICROARCH.md section HBM)',
        'conv_family': {'kernels': sorted(set(k['kernel'] for k in fam)), 'launches': n,
                        'hbm_bytes_per_launch_corrected': int(sum(k['hbm_bytes_per_launch_corrected'] * k['launches'] for k in fam) / max(n, 1))},
        'kernels': kernels[:60],
    }
    f44 = [k for k in kernels if k['kernel'].startswith('wino44_conv_kernel')]     # the launches routed to Winograd F(4x4,3x3): their own record
    if f44:
        n44 = sum(k['launches'] for k in f44)
        out['conv_family_f4x4'] = {'kernels': sorted(set(k['kernel'] for k in f44)), 'launches': n44,
                                   'hbm_bytes_per_launch_corrected': int(sum(k['hbm_bytes_per_launch_corrected'] * k['launches'] for k in f44) / n44)}
    # optional 4th argument: number of forward passes the profiled command ran (FlowNet2: every pass is the same work) -> whole-run
    # HBM bytes per pass.  A UNet bench process is NOT uniform (train steps + forward-only passes + one-off set-up), so for it the
    # per-step total is derived from the once-per-step kernels: train steps = launches of adam_bucketed_kernel, forward passes =
    # launches of outconv_fwd_kernel / outconv_fwdbwd_kernel / outconv8_kernel<., 0 | 2, ..>; only a process that ran train steps ALONE (bench.py --no-forward-timing) yields a per-step
    # total (round 3 divided a 6-train-step + 10-forward-pass process by `runs` = 5: VERDICT r3 weak #6).
    tot = sum((2 * fetch[k] + write.get(k, 0.0)) * 1024 for k in fetch)
    n_adam = sum(n for k, n in nf.items() if k.startswith('adam_bucketed_kernel'))
    import re as _re
    # (outconv8_kernel<CC, MODE, ...>: MODE 0 = forward, 2 = forward + backward, 1 = backward only)
    n_fwd = sum(n for k, n in nf.items() if k.startswith('outconv_fwd_kernel') or k.startswith('outconv_fwdbwd_kernel')
                or _re.match(r'outconv8_kernel<\d+, [02],', k))
    if n_adam and n_fwd:
        out['train_steps_profiled'] = n_adam
        out['forward_passes_profiled'] = n_fwd
        if n_fwd == n_adam:       # the process ran train steps only (bench.py --no-forward-timing): the total IS per-step
            out['hbm_bytes_per_train_step'] = int(tot / n_adam)
        else:
            out['hbm_bytes_per_train_step'] = None
            out['note_per_step'] = ('the profiled process ran %d train steps and %d forward passes (%d forward-only): its total is '
                                    'not a per-step figure; profile with bench.py --no-forward-timing' % (n_adam, n_fwd, n_fwd - n_adam))
    if len(sys.argv) > 4:
        n_runs = int(sys.argv[4])
        out['runs'] = n_runs
        out['total_hbm_bytes_per_run_corrected'] = int(tot / n_runs)
    # the library build the counters were taken on (content hash of the kernel sources): bench.py reports a mismatch as STALE
    try:
        import os
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from vec_vad_amd import build as _B
        out['library_build'] = _B.wanted()[1][:16]
    except Exception:
        out['library_build'] = None
    json.dump(out, open(sys.argv[3], 'w'), indent=1)
    print(json.dumps(out['conv_family']))


if __name__ == '__main__':
    main()
