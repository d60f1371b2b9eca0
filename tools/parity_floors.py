#!/usr/bin/env python3
"""Measures, with the numpy oracle alone, what every solve-against-oracle comparison of the GPU tests compares: the share of
scenarios outside the set-asides, how many of those are solved, their distinct winners and how many cross a curvature
break-point.  tests/golden/parity_floors.json records the figures (compare_solve takes its floors from there) and
tests/test_parity_floors_host.py holds them to the inputs.

    tools/parity_floors.py            print the table
    tools/parity_floors.py --write    ... and rewrite the JSON (the 'why' notes of existing entries are kept)
    tools/parity_floors.py --only fuzz --jobs 8
"""
import argparse
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'igt-mpc-int_amd'), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
PATH = os.path.join(ROOT, 'tests', 'golden', 'parity_floors.json')


def _one(key):
    import parity_cases
    return parity_cases.measure_key(key)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--write', action='store_true')
    ap.add_argument('--only', default='', help='substring of the case keys to measure')
    ap.add_argument('--jobs', type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    import parity_cases
    keys = [k for k, _ in parity_cases.all_cases() if a.only in k]
    old = {}
    if os.path.exists(PATH):
        with open(PATH) as fh:
            old = json.load(fh)['cases']
    new = {} if not a.only else dict(old)
    with ProcessPoolExecutor(a.jobs) as ex:
        for res in ex.map(_one, keys):
            for k, m in res.items():
                e = dict(B=m['B'], compared=m['compared'], tie_compared=m['tie_compared'], solved=m['solved'],
                         min_solved=parity_cases.min_solved_for(m['solved']), winners=m['winners'], crossing=m['crossing'])
                if 'why' in old.get(k, {}):
                    e['why'] = old[k]['why']
                new[k] = e
                flag = '' if m['solved'] >= m['need'] and m['crossing'] >= m['crossing_needed'] else '   <-- below what the case needs'
                print(f'{k:44s} B {m["B"]:4d}  compared {m["compared"]:4d}  outside edges {m["tie_compared"]:4d}  solved {m["solved"]:4d}  '
                      f'winners {m["winners"]:3d}  crossing {m["crossing"]:3d}{flag}', flush=True)
    if a.write:
        doc = dict(note='CPU-measured figures of the solve-against-oracle comparisons (tools/parity_floors.py --write). share = '
                        'compared / B, asserted less one scenario or 0.02; min_solved = solved less a tenth. why: the reason '
                        'for a float64 share below 1.', cases=new)
        with open(PATH, 'w') as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
            fh.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
