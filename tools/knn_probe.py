"""Per-call time of the cosine top-k per shape (HIP events per call):
  python3 tools/knn_probe.py                      1M x 64, k = 11, Q = 1 .. 256, then an
                                                  agreement check against a torch brute force
  python3 tools/knn_probe.py --N 3000 20000 60000 --Q 1 32 --repeat 20
                                                  the small tables (the reference's own hotel
                                                  counts are in the thousands)
  python3 tools/knn_probe.py --N 1430000 --Q 256 --dups 5000
                                                  every query's list overflowed (the table of
                                                  test_cosine_knn_v4_batched_fallback, every = 1)
--N --d --k --Q take lists (every combination is timed); DCNR_LIB selects the library."""
import argparse, os, sys, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "hybrid-hotel-recommendation-system-based-on-friends-recommendations_amd"))
import dcnr
from dcnr import _lib
DEFAULT_Q = [1, 2, 4, 8, 16, 32, 256]
ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, nargs="+", default=[1_000_000])
ap.add_argument("--d", type=int, nargs="+", default=[64])
ap.add_argument("--k", type=int, nargs="+", default=[11])
ap.add_argument("--Q", type=int, nargs="+", default=DEFAULT_Q)
ap.add_argument("--repeat", type=int, default=10)
ap.add_argument("--dups", type=int, default=0,
                help="random queries, each with this many scaled copies planted in the table")
args = ap.parse_args()
default = (args.N, args.d, args.k, args.Q, args.dups) == ([1_000_000], [64], [11], DEFAULT_Q, 0)
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
for N in args.N:
    for d in args.d:
        tab = torch.randn((N, d), generator=g, device=dev)
        nn = dcnr.NearestNeighbors(metric="cosine").fit(tab)
        for k in args.k:
            for Q in args.Q:
                if args.dups:
                    tab = torch.randn((N, d), generator=g, device=dev)
                    q = torch.randn((Q, d), generator=g, device=dev)
                    perm = torch.randperm(N, generator=g, device=dev)
                    for j in range(Q):
                        tab[perm[args.dups * j:args.dups * (j + 1)]] = q[j] * (0.5 + j % 3)
                    nn = dcnr.NearestNeighbors(metric="cosine").fit(tab)
                else:
                    q = tab[torch.randint(0, N, (Q,), generator=g, device=dev)]
                for _ in range(3): nn.kneighbors_device(q, k)
                torch.cuda.synchronize()
                _lib.profile_enable(True); _lib.profile_collect()
                for _ in range(args.repeat): nn.kneighbors_device(q, k)
                _lib.profile_enable(False)
                ms, cnt = _lib.profile_collect()["knn"]
                ms /= args.repeat
                if default:
                    print(f"Q={Q}: {ms*1e3:.1f} us per call ({cnt/args.repeat:.0f} launches), "
                          f"{260e6/(ms/1e3)/1e9:.0f} GB/s of table")
                else:
                    print(f"N={N} d={d} k={k} Q={Q}: {ms*1e3:.1f} us per call")
if default:
    # agreement with a torch fp32 brute force on a few queries (index sets, distances)
    tn = tab / tab.norm(dim=1, keepdim=True)
    for Q in (8, 4, 40, 300):
        q = tab[torch.randint(0, 1_000_000, (Q,), generator=g, device=dev)]
        d, i = nn.kneighbors_device(q, 11)
        qn = q / q.norm(dim=1, keepdim=True)
        rd, ri = torch.topk((1 - qn @ tn.T).clamp(0, 2), 11, dim=1, largest=False)
        print(*([] if Q == 8 else [f"Q={Q}:"]), "max |dist diff|", float((rd - d).abs().max()), "same sets",
              sum(set(a.tolist()) == set(b.tolist()) for a, b in zip(i, ri)), f"/ {Q}")
