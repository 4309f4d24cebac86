"""Is any public Y'CbCr operator slower than at another commit?  Runs scripts/bench_yuv.py (this file's neighbour, so both trees are timed
by the same code) against a checkout of that commit and against this tree ALTERNATELY, one fresh process per run and leg - legs (a)
`--skip-video` and (d) `--formats` - and compares every arm with the same call at the other commit:

  per arm    the median of each process is one sample; `parent_us` / `branch_us` are the medians of those samples;
  margin     the spread (max - min) of the PARENT's own samples of that arm - what two runs of the same code differ by;
  within     branch_us <= parent_us + margin.

The other checkout needs its library built (`python -m edvr_amd.build` there).  A run that fails or outlasts its limit ends the whole
comparison: nothing more is started on the device.

    git worktree add ../parent HEAD~1 && (cd ../parent && python -m edvr_amd.build)
    python scripts/bench_yuv_compare.py --parent ../parent [--runs 5] [--out profiles/yuv/bench_yuv_one_family.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
LEGS = {'a': ['--skip-video'], 'd': ['--formats']}


def arms(record):
    """(arm, case) -> the process's median in microseconds, for either leg's record."""
    out = {}
    for row in record.get('kernels', []):
        for key, value in row.items():
            if key.endswith('_us') and not key.startswith('stock'):
                out[('yuv420 ' + key[:-3], row['case'])] = value
    for row in record.get('formats', []):
        pair = 'yuv420' if 'yuv420' in row['ops'] else 'yuv'
        for direction in ('decode', 'encode'):
            out[(f"{pair} {direction} '{row['format']}'", row['case'])] = row[direction + '_us']
    return out


def compare(parent, branch):
    """parent, branch: lists of arms() dicts, one per process -> the comparison rows."""
    rows = []
    for arm, case in parent[0]:
        p, b = [run[(arm, case)] for run in parent], [run[(arm, case)] for run in branch]
        pm, bm, margin = statistics.median(p), statistics.median(b), max(p) - min(p)
        rows.append(dict(arm=arm, case=case, parent_us_runs=p, branch_us_runs=b, parent_us=round(pm, 2), branch_us=round(bm, 2),
                         margin_us=round(margin, 2), branch_minus_parent_us=round(bm - pm, 2), within_margin=bm <= pm + margin))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True, help='a built checkout of the commit to compare against')
    ap.add_argument('--runs', type=int, default=5, help='processes per tree and leg (at least 3)')
    ap.add_argument('--out', default=os.path.join(HERE, '..', 'profiles', 'yuv', 'bench_yuv_one_family.json'))
    ap.add_argument('--parent-head', default=None, help='its commit, where the checkout is not a git one')
    ap.add_argument('--head', default=None, help="this tree's commit, likewise")
    ap.add_argument('--limit', type=int, default=300, help='seconds one process may take')
    args = ap.parse_args()
    assert args.runs >= 3, 'a spread needs at least three runs'
    trees = {'parent': (os.path.abspath(args.parent), args.parent_head), 'branch': (os.path.abspath(os.path.join(HERE, '..')), args.head)}
    records = {name: {leg: [] for leg in LEGS} for name in trees}
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(args.runs):
            for leg, flags in LEGS.items():
                for name, (tree, head) in trees.items():
                    out = os.path.join(tmp, f'{name}_{leg}_{i}.json')
                    cmd = [sys.executable, os.path.join(HERE, 'bench_yuv.py'), '--tree', tree, '--out', out] + flags + (['--head', head] if head else [])
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
                    if r.returncode != 0:
                        raise SystemExit(f'{name} leg ({leg}) run {i} failed with {r.returncode}; nothing more is started\n{r.stdout[-1500:]}{r.stderr[-1500:]}')
                    records[name][leg].append(json.load(open(out)))
            print(f'round {i + 1} of {args.runs} done', flush=True)
    rows = [row for leg in LEGS for row in compare([arms(r) for r in records['parent'][leg]], [arms(r) for r in records['branch'][leg]])]
    first = {name: records[name]['a'][0] for name in trees}
    record = dict(bench='bench_yuv_one_family', script=f'scripts/bench_yuv_compare.py --runs {args.runs}: scripts/bench_yuv.py --skip-video / --formats per process',
                  device=first['branch']['device'], warmup=first['branch']['warmup'], iters=first['branch']['iters'], runs=args.runs,
                  parent={k: first['parent'][k] for k in ('git_head', 'source_hash', 'lib')}, branch={k: first['branch'][k] for k in ('git_head', 'source_hash', 'lib')},
                  margin='per arm: max - min of the parent medians over its runs; within_margin: branch_us <= parent_us + margin_us', comparison=rows)
    for row in rows:
        print(f"{row['arm']:28s} {row['case']:12s} parent {row['parent_us']:7.2f}  branch {row['branch_us']:7.2f}  margin {row['margin_us']:5.2f}  "
              f"{row['branch_minus_parent_us']:+6.2f} {'ok' if row['within_margin'] else 'OVER'}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
    print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
