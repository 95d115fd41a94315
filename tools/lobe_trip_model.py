#!/usr/bin/env python3
"""The trip policy of the role-sorted spheres kernel replayed on the CPU: what lobe-uniform shading trips cost against mixed ones.

    python tools/lobe_trip_model.py [--policy single|lobe|both] [--entries 120,144,168,192] [--ggx-share 0.5,0.65,0.8]
        [--gen 350] [--shade-mixed 700] [--ggx-only 130] [--diffuse-only 30] [--extra-trip 0] [--extra-shade 0] [--gen-credit 0]

A wave's work item is --gen-trips generation trips of 64 (pixel, sample) pairs.  A primary hit parks with probability --park-primary, a shaded
hit parks again with --park-again until a path has been shaded --max-shaded times (0.65 / 0.5 / 3: the 2.13 segments and 1.13 shaded hits per
sample of DESIGN.md section 5.1).  A parked hit's next bounce samples the GGX lobe with probability --ggx-share, independently.

  single  today's rule before the two-ended stack: one stack of --single-entries; a generation trip while the item has pairs and the stack holds at most
          entries - 64 hits, else a shading trip of the top min(n, 64) — every shading trip runs both lobes' streams: --shade-mixed.
  lobe    raymond_amd/csrc/lobe_trips.hpp: two stacks in one array of `entries`; a generation trip while n_d + n_g <= entries - 64, else a
          shading trip of the fuller stack.  A diffuse trip costs shade-mixed - ggx-only, a GGX trip shade-mixed - diffuse-only.  The form's own
          costs: --extra-trip per trip (the second ballot / mbcnt of the push), --extra-shade per shading trip (the normal made again from the
          popped hit point), less --gen-credit per generation trip (the normal that classification no longer makes for a hit it parks).

Costs are vector instructions per trip; a trip costs the same for one lane as for 64.  Prints, per entry count and GGX share, the lobe policy's
cost against the single stack's and the lanes per shading trip."""
import argparse
import random

ap = argparse.ArgumentParser()
ap.add_argument("--policy", default="both")
ap.add_argument("--entries", default="120,144,168,192")
ap.add_argument("--single-entries", type=int, default=120)
ap.add_argument("--ggx-share", default="0.5,0.65,0.8")
ap.add_argument("--gen-trips", type=int, default=167)
ap.add_argument("--items", type=int, default=24)
ap.add_argument("--park-primary", type=float, default=0.65)
ap.add_argument("--park-again", type=float, default=0.5)
ap.add_argument("--max-shaded", type=int, default=3)
ap.add_argument("--gen", type=float, default=350.0)
ap.add_argument("--shade-mixed", type=float, default=700.0)
ap.add_argument("--ggx-only", type=float, default=130.0)
ap.add_argument("--diffuse-only", type=float, default=30.0)
ap.add_argument("--extra-trip", type=float, default=0.0)
ap.add_argument("--extra-shade", type=float, default=0.0)
ap.add_argument("--gen-credit", type=float, default=0.0)
ap.add_argument("--seed", type=int, default=1)
a = ap.parse_args()


def run_item(policy, entries, share, rng):
    """One work item: returns (cost, shading trips, shaded lanes, trips by kind)."""
    stacks = ([], [])  # diffuse, GGX: each entry the number of times its path has been shaded
    pairs = a.gen_trips * 64
    cost, s_trips, s_lanes = 0.0, 0, 0
    kinds = [0, 0, 0]  # generation, diffuse (single: mixed), GGX

    def park(shaded):
        g = 1 if (policy == "lobe" and rng.random() < share) else 0
        stacks[g].append(shaded)

    while True:
        n_d, n_g = len(stacks[0]), len(stacks[1])
        if pairs > 0 and n_d + n_g + 64 <= entries:
            pairs -= 64
            kinds[0] += 1
            cost += a.gen + (a.extra_trip - a.gen_credit if policy == "lobe" else 0.0)
            for _ in range(64):
                if rng.random() < a.park_primary:
                    park(0)
            continue
        if n_d + n_g == 0:
            break
        g = 1 if n_g > n_d else 0
        st = stacks[g]
        n = min(len(st), 64)
        popped = st[len(st) - n:]
        del st[len(st) - n:]
        s_trips += 1
        s_lanes += n
        kinds[1 + g] += 1
        if policy == "lobe":
            cost += a.shade_mixed - (a.diffuse_only if g else a.ggx_only) + a.extra_trip + a.extra_shade
        else:
            cost += a.shade_mixed
        for shaded in popped:
            if shaded + 1 < a.max_shaded and rng.random() < a.park_again:
                park(shaded + 1)
    assert len(stacks[0]) + len(stacks[1]) == 0
    return cost, s_trips, s_lanes, kinds


def run(policy, entries, share):
    rng = random.Random(a.seed)
    tot = [0.0, 0, 0, [0, 0, 0]]
    for _ in range(a.items):
        c, t, l, k = run_item(policy, entries, share, rng)
        tot[0] += c
        tot[1] += t
        tot[2] += l
        tot[3] = [x + y for x, y in zip(tot[3], k)]
    return tot


print("arms: generation %g, mixed shading %g, GGX-only stream %g, diffuse-only stream %g; the lobe form's own: +%g per trip, +%g per shading trip, -%g per generation trip"
      % (a.gen, a.shade_mixed, a.ggx_only, a.diffuse_only, a.extra_trip, a.extra_shade, a.gen_credit))
shares = [float(x) for x in a.ggx_share.split(",")]
if a.policy in ("single", "both"):
    base = run("single", a.single_entries, 0.0)
    print("single stack, %d entries: cost %.0f per item, %.1f lanes per shading trip" % (a.single_entries, base[0] / a.items, base[2] / max(base[1], 1)))
if a.policy in ("lobe", "both"):
    print("| Entries | " + " | ".join("GGX share %.2f: cost against single, lanes per shading trip, diffuse / GGX trips" % s for s in shares) + " |")
    print("|---|" + "---|" * len(shares))
    for e in [int(x) for x in a.entries.split(",")]:
        cells = []
        for s in shares:
            r = run("lobe", e, s)
            rel = (" %+.1f %%" % (100.0 * (r[0] / base[0] - 1.0))) if a.policy == "both" else " %.0f" % (r[0] / a.items)
            cells.append("%s, %.1f, %d / %d" % (rel, r[2] / max(r[1], 1), r[3][1] // a.items, r[3][2] // a.items))
        print("| %d | " % e + " | ".join(cells) + " |")
