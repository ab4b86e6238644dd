"""F11: what the REFERENCE service (main.py:170-357) reads of the reviews and
the friend graph, on a small synthetic dataset with the cases F7 lacks,
produced by running the reference's own functions here (build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_friends_golden.py

Writes tests/golden/f11_friends/ in F7's layout (data/*.csv, artifacts.json,
item_embeddings.npy, expected.json), the model's state_dict as plain arrays
(model_state.npz).  Per request
expected.json records get_friends_for_user's set, the positives and negatives
_generate_candidates derives (its locals ``positive_recs`` and
``negative_filter``, read from the function's frame as it returns: the
function itself runs unchanged), the ranked hotel ids and every
``recommended_by`` list of the /recommendations response.

Planted, besides F7's kinds of requests:
  * friend 112 reviews hotel H twice with >= 8 and friend 111's >= 8 review of
    H lies between the two rows: recommended_by(H) = [112, 111]
  * (113, H3) has a 9 and a 2: H3 is positive AND negative for 113's friends
  * friendships (110, 110), (110, 111) twice, (111, 110)
  * ratings of exactly 8 and exactly 4
  * user 120's only friends (105, 106) have no reviews; user 121 has no
    friends; user 9999 is unknown
  * both modes
"""
from __future__ import annotations

import json
import os
import shutil
import sys
import tempfile

import numpy as np
import pandas as pd
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import golden_common as gc  # noqa: E402
from make_request_golden import CAT_COLS, CITIES, NUM_COLS, PARAMS  # noqa: E402
from make_serving_golden import load_main  # noqa: E402

OUT = os.path.join(HERE, "f11_friends")
N_GUESTS, N_HOTELS = 60, 80
NO_REVIEWS = (5, 6)            # guests 105, 106
H, H2, H3, H4, H5 = 3, 6, 9, 12, 15    # hotel indices, all in CITIES[0]


def make_data(rng):
    hotels = pd.DataFrame({
        "hotel_id": 500 + 7 * np.arange(N_HOTELS),
        "city": [CITIES[i % 3] for i in range(N_HOTELS)],
        "price_rub": rng.integers(2000, 20000, N_HOTELS).astype(float),
        "stars": rng.integers(1, 6, N_HOTELS).astype(float),
        "hotel_type": rng.choice(["hotel", "hostel", "apart", "resort"], N_HOTELS),
        "district": rng.choice(["center", "north", "south", "east", "west", "port"], N_HOTELS),
        "user_reviews_count": rng.integers(0, 500, N_HOTELS),
    })

    def review(g, h, overall):
        r = dict(hotels.iloc[h])
        r["guest_id"] = 100 + g
        r["rating_overall"] = int(overall)
        r["rating_cleanliness"] = float(rng.integers(1, 11))
        r["rating_service"] = float(rng.integers(1, 11))
        r["rating_location"] = float(rng.integers(1, 11))
        return r

    planted_hotels = {H, H2, H3, H4, H5}
    rows = []
    for g in range(N_GUESTS):
        if g in NO_REVIEWS:
            continue
        free = [h for h in range(N_HOTELS) if h not in planted_hotels]
        for h in rng.choice(free, rng.integers(3, 9), replace=False):
            rows.append(review(g, int(h), rng.integers(1, 11)))
    main = pd.DataFrame(rows).sample(frac=1.0, random_state=5).reset_index(drop=True)
    # planted rows keep their order: spliced into the shuffled table at fixed places
    planted = [(40, review(12, H, 9)), (90, review(11, H, 8)), (150, review(12, H, 10)),
               (60, review(13, H3, 9)), (200, review(13, H3, 2)),
               (120, review(12, H4, 8)), (130, review(12, H5, 4)),
               (20, review(11, H2, 10)), (220, review(10, H2, 8)), (230, review(10, H5, 3))]
    for at, r in sorted(planted, key=lambda p: p[0]):
        main = pd.concat([main.iloc[:at], pd.DataFrame([r]), main.iloc[at:]], ignore_index=True)
    pairs = set()
    while len(pairs) < 90:
        a, b = rng.integers(0, N_GUESTS, 2)
        if a != b and 20 not in (a, b) and 21 not in (a, b) and not {int(a), int(b)} & set(NO_REVIEWS):
            pairs.add((100 + int(min(a, b)), 100 + int(max(a, b))))
    pairs = sorted(pairs) + [(110, 110), (110, 111), (110, 111), (111, 110), (110, 112),
                             (113, 110), (120, 105), (106, 120)]
    friends = pd.DataFrame(pairs, columns=["user_id_1", "user_id_2"])
    return main, friends


REQUESTS = [(110, CITIES[0], "friends", 1.0), (110, CITIES[0], "personal", 1.0),
            (110, CITIES[0], "friends", 0.3), (111, CITIES[0], "friends", 0.7),
            (112, CITIES[0], "personal", 0.7), (113, CITIES[0], "friends", 1.0),
            (120, CITIES[1], "friends", 0.7), (121, CITIES[1], "friends", 1.0),
            (121, CITIES[2], "personal", 0.3), (9999, CITIES[0], "friends", 0.7),
            (9999, CITIES[2], "personal", 1.0), (131, CITIES[1], "friends", 0.5),
            (131, CITIES[1], "personal", 0.0), (142, CITIES[2], "friends", 1.0),
            (105, CITIES[0], "personal", 0.7), (150, "Atlantis", "friends", 0.7)]


def main():
    ref = load_main()
    rng = np.random.default_rng(1111)
    main_df, friends = make_data(rng)
    feat = main_df.rename(columns={"guest_id": "user_id", "hotel_id": "item_id"})
    feat["price_per_star"] = (feat["price_rub"] / feat["stars"]).replace([np.inf, -np.inf], 0).fillna(0)
    feat["cleanliness_vs_service"] = (feat["rating_cleanliness"] / feat["rating_service"]).replace(
        [np.inf, -np.inf], 0).fillna(0)
    feat["location_premium"] = feat["rating_overall"] - feat["rating_location"]
    users = sorted(feat["user_id"].unique().tolist()) + [100 + g for g in NO_REVIEWS]
    items = sorted(feat["item_id"].unique().tolist())
    user_map = {int(u): i for i, u in enumerate(users)}
    item_map = {int(h): i for i, h in enumerate(items)}
    encoders = {c: {v: i for i, v in enumerate(sorted(feat[c].unique()))} for c in CAT_COLS}
    from sklearn.preprocessing import MinMaxScaler
    scaler = MinMaxScaler().fit(feat[NUM_COLS])
    cat_dims = {c: len(e) for c, e in encoders.items()}

    torch.manual_seed(11)
    model = ref.DCN_RecSys(len(user_map), len(item_map), cat_dims, len(NUM_COLS), dict(PARAMS))
    gc.perturb_state(model, 12)
    model.eval()

    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(os.path.join(OUT, "data"))
    main_df.to_csv(os.path.join(OUT, "data", "hackathon_augmented_data.csv"), index=False)
    friends.to_csv(os.path.join(OUT, "data", "friendships.csv"), index=False)
    # the weights as plain arrays (state_dict order kept); the .pth the reference
    # loads is written to the temp dir only
    np.savez(os.path.join(OUT, "model_state.npz"),
             **{k: v.detach().cpu().numpy() for k, v in model.state_dict().items()})
    np.save(os.path.join(OUT, "item_embeddings.npy"),
            model.item_embedding.weight.detach().cpu().numpy())
    with open(os.path.join(OUT, "artifacts.json"), "w") as f:
        json.dump({"user_id_mapping": {str(k): v for k, v in user_map.items()},
                   "item_id_mapping": {str(k): v for k, v in item_map.items()},
                   "cat_encoders": encoders, "numerical_cols": NUM_COLS,
                   "scaler_min": scaler.min_.tolist(), "scaler_scale": scaler.scale_.tolist(),
                   "model_dims": [len(user_map), len(item_map), cat_dims, len(NUM_COLS)],
                   "best_params": PARAMS}, f, indent=1)

    import joblib
    seen = {}

    def on_return(frame, event, arg):   # the locals of _generate_candidates as it returns
        if event == "return" and frame.f_code.co_name == "_generate_candidates":
            seen["pos"] = [int(h) for h in frame.f_locals["positive_recs"]]
            seen["neg"] = sorted(int(h) for h in frame.f_locals["negative_filter"])

    expected = {"recommendations": [], "similar_items": []}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copytree(os.path.join(OUT, "data"), os.path.join(tmp, "data"))
        art = os.path.join(tmp, "artifacts")
        os.makedirs(art)
        joblib.dump({"user_id_mapping": user_map, "item_id_mapping": item_map,
                     "cat_encoders": encoders, "numerical_cols": NUM_COLS, "scaler": scaler},
                    os.path.join(art, "artifacts.gz"))
        joblib.dump((len(user_map), len(item_map), cat_dims, len(NUM_COLS)),
                    os.path.join(art, "model_dims.gz"))
        joblib.dump(dict(PARAMS), os.path.join(art, "best_params.gz"))
        shutil.copy(os.path.join(OUT, "item_embeddings.npy"), art)
        torch.save(model.state_dict(), os.path.join(art, "final_dcn_model.pth"))
        os.chdir(tmp)
        try:
            ref.load_artifacts()
            for uid, city, mode, lam in REQUESTS:
                seen.clear()
                sys.setprofile(on_return)
                try:
                    r = ref.get_recommendations_endpoint(ref.RecommendationRequest(
                        user_id=uid, city=city, type=mode, lambda_param=lam))
                finally:
                    sys.setprofile(None)
                expected["recommendations"].append({
                    "user_id": uid, "city": city, "type": mode, "lambda_param": lam,
                    "friends": sorted(int(x) for x in ref.get_friends_for_user(uid)),
                    "positives": seen["pos"], "negatives": seen["neg"],
                    "ranked_hotels": [int(h["hotel_id"]) for h in r["ranked_hotels"]],
                    "recommended_by": [[int(x) for x in h["recommended_by"]]
                                       for h in r["ranked_hotels"]],
                    "message": r.get("message")})
        finally:
            os.chdir(cwd)
    with open(os.path.join(OUT, "expected.json"), "w") as f:
        json.dump(expected, f, indent=1)
    for r in expected["recommendations"]:
        print(r["user_id"], r["city"], r["type"], r["lambda_param"], len(r["friends"]),
              len(r["positives"]), len(r["negatives"]), len(r["ranked_hotels"]),
              sum(len(b) for b in r["recommended_by"]), r["message"])
    print("wrote", sorted(os.listdir(OUT)))


if __name__ == "__main__":
    main()
