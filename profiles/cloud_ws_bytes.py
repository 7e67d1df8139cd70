#!/usr/bin/env python3
"""Device bytes of the cloud stages' workspace after lfd_consensus_filter, lfd_fuse_oriented, lfd_knn_dist2 and lfd_voxel_downsample have each
run once on a cloud of n points (and, with --freespace, lfd_freespace_filter too): five grow-only buffers before the stages shared one
(their sum), one buffer since (the largest).  Computed from n with the plan's own formulas (csrc/lfd_api.hip: cloud_plan, carve_sort, the
stages' layouts) - every region rounded up to 256 bytes, the buffer too; no GPU needed.

    python profiles/cloud_ws_bytes.py 34532088 --refs 148                          # the dense-mode cloud of profiles/consensus_time.py
    python profiles/cloud_ws_bytes.py 34532088 --refs 148 --freespace 512 332      # ... with the free-space filter's z-buffers of 512 x 332 cells
"""
import argparse

STATS, PT, CAM, BIG = 32, 16, 112, 64       # sizeof LfdVoxStats, LfdConsensusPt = LfdKnnPt, LfdFreespaceCam; LFD_VOX_BIG


def al(b):
    return (b + 255) & ~255


def sort_regions(n, counters, heads):
    r = [1024 * STATS, STATS + 4 * counters, 256 * 1024 * 4, 8 * n, 8 * n, 4 * n, 4 * n]
    return r + ([4 * n] if heads else [])


def compact_regions(n, refs):
    n_wg = (n + 255) // 256
    return [8 * (refs + 1), 8 * (refs + 1), n_wg * 256, 4 * (n_wg + 1)]


def stages(n, refs, plane):
    big = 4 * (n // (BIG + 1) + 1)
    s = {"voxel": sort_regions(n, 2, True) + [big],
         "consensus": sort_regions(n, 0, False) + [PT * n] + compact_regions(n, refs),
         "fuse": sort_regions(n, 3, True) + [4 * n, big, n],
         "knn": sort_regions(n, 3, True) + [PT * n, 4 * n]}
    if plane:
        s["freespace"] = [4 * refs * plane[0] * plane[1], CAM * refs] + compact_regions(n, refs)
    return {k: sum(al(b) for b in v) for k, v in s.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("--refs", type=int, default=148)
    ap.add_argument("--freespace", type=int, nargs=2, default=None, metavar=("PW", "PH"))
    a = ap.parse_args()
    b = stages(a.n, a.refs, a.freespace)
    for k, v in b.items():
        print(f"{k:<10} {v:>15,} bytes  {v / a.n:6.2f} per point")
    print(f"five buffers (before): {sum(b.values()):>15,} bytes = {sum(b.values()) / 2 ** 20:9.1f} MiB")
    print(f"one buffer  (since):   {max(b.values()):>15,} bytes = {max(b.values()) / 2 ** 20:9.1f} MiB")


if __name__ == "__main__":
    main()
