#!/usr/bin/env python3
"""CPU model of the matrix phase of predict_fused_kernel's skipping instances (eight waves x 64
draws, csrc/fused_skip.h) on the benchmark's table and draws: how much matrix work every (tile,
part) job keeps once all-zero density blocks are left out, what that puts on each SIMD under the
kernel's pairing of parts, and what is left of the busiest SIMD when the last r pass is handed
out through a queue (option "fused_share", profiles/share_notes.md).  NumPy only, no device.

    python tools/fused_share_model.py [--seed 1] [--draws 10000] [--n-prim 50] [--n-r 19]
                                      [--overhead 0 2]

The kernel's rules, as the model uses them:
  * 2 n_prim density rows (centrals, then satellites) in blocks of four; the triangle of block
    pairs cut into four parts of equal numbers of units (hostmath.cpp: triangle_parts);
  * a satellite bin is exactly zero for a draw whose M0 lies at or above the bin's highest
    quadrature node (ten Gauss-Legendre nodes in log mass);
  * a workgroup's 64 draws ranked by M0 (NaN first, ties by index), ranks 16 g .. 16 g + 15 form
    group g, groups 0 / 1 are tile 0, 2 / 3 tile 1; the last workgroup is filled with copies of the
    batch's last draw;
  * a product (unit, group) is left out where the unit's block column or block row is zero for
    all 16 draws of the group: the cost of a job is what remains, in units x groups;
  * waves w and w + 4 share SIMD w and take the parts (0, 1), (2, 3), (1, 0), (3, 2).
Assumptions of the schedule: the two waves of a SIMD share its matrix pipe equally, an item
costs its products plus `overhead` units, the co-resident workgroup does not interfere, and the r
passes of a job cost in proportion to their sub-tiles (U = 5: 2, 2, 1).
"""

import argparse

import numpy as np

LOW = np.array([11.5, 0.1, 11.0, 12.5, 0.7])       # tabcorr_amd/synthetic.py: zheng07_draws
HIGH = np.array([13.5, 0.8, 13.0, 14.5, 1.4])
PARTS = 4
# part of wave w (tile 0) and of wave w + 4 (tile 1) on SIMD w
PAIRING = [(0, 1), (2, 3), (1, 0), (3, 2)]
ITEM_PARTS = (0, 3, 2, 1)                          # fused_skip.h: share_item


def triangle_parts(n_rb, n_parts):
    n_units = n_rb * (n_rb + 1) // 2
    parts = []
    for part in range(n_parts):
        begin, end = n_units * part // n_parts, n_units * (part + 1) // n_parts
        units, rb, cb = [], 0, 0
        for index in range(end):
            if index >= begin:
                units.append((rb, cb))
            cb += 1
            if cb > rb:
                rb, cb = rb + 1, 0
        parts.append(units)
    return parts


def job_costs(log_m0, n_prim, log_m_min=10.5, log_m_max=15.0):
    """(workgroups, tile, part, group) products that remain, in units."""
    edges = np.linspace(log_m_min, log_m_max, n_prim + 1)
    top_node = (np.polynomial.legendre.leggauss(10)[0][-1] + 1) / 2
    highest = edges[:-1] + (edges[1:] - edges[:-1]) * top_node      # per satellite bin
    n_rows = (2 * n_prim + 3) // 4 * 4
    n_blocks = n_rows // 4
    parts = triangle_parts(n_blocks, PARTS)
    n_draws = len(log_m0)
    n_wg = (n_draws + 63) // 64
    costs = np.zeros((n_wg, 2, PARTS, 2))
    for wg in range(n_wg):
        index = np.minimum(np.arange(64) + 64 * wg, n_draws - 1)
        m0 = log_m0[index]
        key = np.where(np.isnan(m0), -np.inf, m0)
        order = np.argsort(key, kind='stable')
        for g in range(4):
            lowest = key[order[16 * g]]            # the group's smallest M0
            zero_row = np.zeros(n_rows, dtype=bool)
            zero_row[n_prim:2 * n_prim] = highest <= lowest
            zero_row[2 * n_prim:] = True           # padding rows
            zero_block = zero_row.reshape(n_blocks, 4).all(axis=1)
            for part, units in enumerate(parts):
                costs[wg, g // 2, part, g % 2] = sum(
                    1 for rb, cb in units if not zero_block[rb] and not zero_block[cb])
    return costs, sum(len(units) for units in parts)


def simulate(own, items, overhead):
    """Eight waves, wave w on SIMD w % 4: each walks `own[w]`, then takes items in order until
    none is left; two waves of a SIMD that both work advance at half speed.  -> makespan."""
    left = np.array(own, dtype=float)
    busy = left > 0
    queue = list(items)
    now = 0.0

    def refill():
        for w in range(8):
            while not busy[w] and queue:
                left[w] = queue.pop(0) + overhead
                busy[w] = left[w] > 0
    refill()
    while busy.any():
        share = np.array([int(busy[w % 4]) + int(busy[w % 4 + 4]) for w in range(8)],
                         dtype=float)
        time_to_end = np.where(busy, left * share, np.inf)
        step = time_to_end.min()
        now += step
        left = np.where(busy, left - step / np.maximum(share, 1.0), left)
        done = busy & (left <= 1e-9)
        busy &= ~done
        left[done] = 0.0
        refill()
    return now


def main():
    parser = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    parser.add_argument('--seed', type=int, default=1)
    parser.add_argument('--draws', type=int, default=10000)
    parser.add_argument('--n-prim', type=int, default=50)
    parser.add_argument('--n-r', type=int, default=19)
    parser.add_argument('--overhead', type=float, nargs='*', default=[0.0, 2.0])
    args = parser.parse_args()
    theta = np.random.default_rng(args.seed).uniform(LOW, HIGH, size=(args.draws, 5))
    costs, n_units = job_costs(theta[:, 2], args.n_prim)
    n_wg = len(costs)
    n_u = (args.n_r + 3) // 4
    passes = [2] * (n_u // 2) + [1] * (n_u % 2)
    last = passes[-1] / sum(passes) if passes[-1] == 1 and n_u > 1 else 0.0
    job = costs.sum(axis=3)                        # (workgroup, tile, part)
    print('%d draws (seed %d), %d workgroups, %d units per tile, U = %d' %
          (args.draws, args.seed, n_wg, n_units, n_u))
    print('matrix instructions kept: %.3f' % (job.sum() / (n_wg * 2 * 2 * n_units)))
    print('mean matrix work per (tile, part), units x groups:')
    for tile in range(2):
        print('  tile %d: ' % tile + '  '.join('%6.1f' % v for v in job[:, tile].mean(axis=0)))
    simd = np.stack([job[:, 0, a] + job[:, 1, b] for a, b in PAIRING], axis=1)
    print('mean load per SIMD: ' + '  '.join('%6.1f' % v for v in simd.mean(axis=0)))
    print('busiest SIMD, mean over the workgroups: %.1f; a perfect split: %.1f' %
          (simd.max(axis=1).mean(), simd.sum(axis=1).mean() / 4))
    if last == 0.0:
        print('the last r pass is not a single sub-tile: nothing to share')
        return
    for overhead in args.overhead:
        spans = {1: [], 2: []}
        for wg in range(n_wg):
            own = np.zeros(8)
            for w, (a, b) in enumerate(PAIRING):
                own[w] = (1 - last) * job[wg, 0, a]
                own[w + 4] = (1 - last) * job[wg, 1, b]
            by_job = [last * job[wg, tile, part] for part in ITEM_PARTS for tile in range(2)]
            by_group = [last * costs[wg, tile, part, g] for part in ITEM_PARTS
                        for tile in range(2) for g in range(2)]
            spans[1].append(simulate(own, by_job, overhead))
            spans[2].append(simulate(own, by_group, overhead))
        print('overhead %.1f units per item: fused_share 1 %.1f, fused_share 2 %.1f '
              '(the last pass is %.2f of a job)' %
              (overhead, np.mean(spans[1]), np.mean(spans[2]), last))


if __name__ == '__main__':
    main()
