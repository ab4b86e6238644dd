"""The requests of F14 (tests/golden/f14_request_pack.npz): what the host half
of the batched request path packs for upload.  Shared by the recorder
(make_request_pack_golden.py) and tests/test_request_pack_cpu.py.

Tables: 40 users, 50 hotel rows, n_neighbors k = 3, two registered sets, and a
city generation of C = 3 cities (its 2C + 1 sets: the cities, their popular
hotels, the empty set of an unknown city)."""
from __future__ import annotations

import numpy as np
import torch

N_USERS, N_ROWS, K = 40, 50, 3
REG_SETS = (np.array([3, 4, 7, 10, 20], np.int64), np.array([0, 1, 2, 48, 49], np.int64))
REG_OFF = np.array([0, 5, 10], np.int64)
N_CITIES = 3
CITY_OFF = np.array([0, 4, 9, 12, 14, 17, 19, 19], np.int64)   # host_offsets of the generation
# rounds to 1.0f from below: < 1 as a double, not as the float32 the kernels compute with
ODD = 1.0 - 2.0 ** -26

U6 = np.array([0, 39, 7, 7, 12, 30], np.int64)
P6 = [[1, 2, 3], [], np.array([49, 0], np.int64), torch.tensor([5, 5, 6, 7]), (10,), range(20, 25)]


def req(users, positives, lambda_param=1.0, top_k=20, allowed=None, excluded=None, fallback=None,
        neighbors_within=None, cities=None, in_city=False):
    return dict(users=np.asarray(users, np.int64).reshape(-1), positive_rows=positives,
                lambda_param=lambda_param, top_k=top_k, allowed=allowed, excluded=excluded,
                fallback=fallback, neighbors_within=neighbors_within, cities=cities,
                in_city=in_city)


def cases():
    """name -> request arguments, R = 1 and R = 6."""
    assert np.float64(ODD) < 1.0 and np.float32(ODD) == np.float32(1.0)
    return {
        "r1_plain": req([5], [[1, 2, 3]]),
        "r1_no_positives": req([0], [[]], 0.7, 5),
        "r1_odd_lambda": req([39], [torch.tensor([4, 4, 9])], ODD, 3),
        "r1_sets": req([5], [[1, 2]], 0.5, 20, allowed=[0], excluded=[[5, 6, 5]], fallback=[1],
                       neighbors_within=[np.array([13, 10, 11, 12])]),
        "r1_all_none": req([5], [[1, 2]], allowed=[None], excluded=[None]),
        "r1_city": req([3], [[8]], 0.9, 20, cities=[1], in_city=True),
        "r1_city_unknown": req([3], [[8]], cities=[-1]),
        "r6_scalars": req(U6, P6, 0.7, 20),
        "r6_per_request": req(U6, P6, [1.0, 0.0, ODD, 0.25, 0.999, 2.0], [1, 2, 3, 20, 128, 7]),
        "r6_sets": req(U6, P6, [0.7, 1.0, ODD, 0.1, 0.5, 1.0], 20,
                       allowed=[None, 0, [9, 8, 8], 1, None, range(15, 30)],
                       excluded=[{4, 2}, None, None, 0, torch.tensor([49]), None],
                       fallback=[1, None, np.array([30, 31, 32, 33, 34, 35, 36]), None, 0, None],
                       neighbors_within=[None, 1, None, [40, 41, 42], None, 0]),
        "r6_all_none": req(U6, P6, 0.7, 20, allowed=[None] * 6, fallback=[None] * 6,
                           neighbors_within=[None] * 6),
        "r6_within_all": req(U6, P6, 0.7, 20, neighbors_within=[0, 1, 0, range(50), 1, [2, 1]]),
        "r6_within_empty_global": req(U6, P6, 0.7, 20, neighbors_within=[0, None, 0, 0, 1, 1]),
        "r6_city": req(U6, P6, 0.7, [20, 20, 3, 3, 1, 1], excluded=[None, [1], None, 1, None, None],
                       cities=[0, -1, 2, 1, -1, 0]),
        "r6_city_neighbors": req(U6, P6, [0.7] * 6, 20, cities=[2, 2, -1, 0, 1, 1], in_city=True),
    }


def errors():
    """name -> (request arguments, the ValueError's text)."""
    return {
        "user": (req([5, 40], [[1], [2]]), "recommend_many: user row outside [0, 40)"),
        "user_negative": (req([-1], [[1]]), "recommend_many: user row outside [0, 40)"),
        "positive": (req([5, 6], [[1], [2, 50]]), "recommend_many: positive row outside [0, 50)"),
        "top_k": (req([5], [[1]], top_k=0), "recommend_many: top_k must be at least 1"),
        "top_k_one_of": (req([5, 6], [[1], [2]], top_k=[3, 0]),
                         "recommend_many: top_k must be at least 1"),
        "length": (req([5, 6], [[1], [2]], fallback=[0]),
                   "recommend_many: fallback needs one entry per request"),
        "unregistered": (req([5, 6], [[1], [2]], allowed=[None, 2]),
                         "recommend_many: allowed[1] = 2 is not a registered set"),
        "unregistered_city": (req([5], [[1]], excluded=[2], cities=[0]),
                              "recommend_many: excluded[0] = 2 is not a registered set"),
        "adhoc_row": (req([5, 6], [[1], [2]], neighbors_within=[None, [3, 50]]),
                      "recommend_many: neighbors_within[1]: row outside [0, 50)"),
    }
