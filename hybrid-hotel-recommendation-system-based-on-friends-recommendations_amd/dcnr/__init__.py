"""dcnr -- MI355X-native (gfx950 HIP) DCN-R ranking path.

Drop-in surfaces of the reference (Krist-Marrakesh/Hybrid-Hotel-Recommendation-
System-Based-on-Friends-Recommendations):

  DCN_RecSys, CrossLayer, ResBlock   train.py:90-170 / main.py:61-127
  BCEWithLogitsLoss                  train.py:206
  AdamW, Adam                        train.py:201-204
  NearestNeighbors (cosine, brute)   main.py:268-270; .build_neighbor_table: every
                                     row's neighbours, computed once;
                                     .kneighbors(within=rows) /
                                     .kneighbors_within_device: the k nearest
                                     rows of a row set (a city's hotels)
  FusedTrainer                       the train.py:219-226 inner-loop step;
                                     .fit: the epoch loop, train.py:216-253
  PlateauLR                          ReduceLROnPlateau (train.py:208-213, 235)
  eval_metrics, roc_auc_score,       BCEWithLogitsLoss / roc_auc_score / RMSE of
  evaluate                           the validation pass (train.py:228-233,
                                     255-265, 366-387)
  group_metrics, evaluate_ranking    per-user (or per-item) GAUC, NDCG@k, hit
                                     rate@k, recall@k and MRR of the order
                                     /recommendations serves (main.py:325)
  list_metrics,                      what the served lists look like under
  popularity_information             lambda_param (main.py:133-169): intra-list
                                     diversity, coverage, Gini, novelty, held-out
                                     hits; RankingPipeline.list_metrics /
                                     .lambda_sweep
  DeviceLoader                       TensorDataset + DataLoader (train.py:195-196)
  serving.rerank_with_mmr            main.py:133-169
  serving.RankingPipeline            the /recommendations + /similar_items core
                                     (main.py:196-230, 294-332); neighbor_table=
                                     serves both from the item neighbour table;
                                     neighbors_within= / within= seek the
                                     neighbours inside the target city instead
                                     of intersecting afterwards (main.py:209-210);
                                     recommend_many answers requests above the
                                     4096-row capacity in the same device pass
                                     (the large lane), recommend()'s MMR takes
                                     any number of candidates
  InteractionStore                   main_df's reviews + friendships_df as the
                                     request path reads them (main.py:172-194,
                                     336-351); RankingPipeline.recommend_users
  CitySets                           a city's hotels and its most reviewed hotels
                                     (main.py:204-210) from main_df's rows, on the
                                     device; recommend_many / recommend_users
                                     (cities=...) name a request's city by code
  ItemFeatures                       each hotel's ranking features from its first
                                     main_df row (main.py:315, 215-230), on the
                                     device; RankingPipeline(item_features=...)
  prepare_data, PreparedData         the driver's filter and derived columns and
                                     prepare_data (train.py:280-287, 36-87) on the
                                     device: raw review columns to the training
                                     tensors, id maps, encoders and scaler;
                                     prepare_data_host: the numpy yardstick
  Preprocessor, Transformed, IdMap   a fitted preprocessing applied to rows it was
                                     not fitted on (preprocess_for_ranking,
                                     main.py:215-230), on the device: raw ids
                                     through a device hash table, category keys,
                                     NaN fill, scaler; PreparedData.preprocessor(),
                                     Preprocessor.from_artifacts; transform_host:
                                     the numpy yardstick
  admission                          a user or hotel the fit has not seen, admitted
                                     in place: IdMap.insert / Preprocessor.admit /
                                     transform(unknown="admit") number the new ids
                                     by first appearance (train.py:42-43);
                                     DCN_RecSys.grow_ and FusedTrainer.grow add
                                     their table rows (moments kept);
                                     NearestNeighbors.append_rows and
                                     RankingPipeline.append_items their index rows
                                     and neighbour lists, as a fresh fit + build
  artifacts.save_artifacts /         final_dcn_model.pth + item_embeddings.npy
  artifacts.load_artifacts           (train.py:391-394, main.py:256-270)
  artifacts.save_neighbor_table /    item_neighbors.npy (+ fingerprint): the
  artifacts.load_neighbor_table      neighbour table beside those files

All compute runs in libdcnr.so (C ABI: include/dcnr.h) on the HIP device.
"""
from .model import CrossLayer, DCN_RecSys, ResBlock  # noqa: F401
from .ops import Adam, AdamW, BCEWithLogitsLoss, bce_with_logits  # noqa: F401
from .knn import NearestNeighbors, ShardedNearestNeighbors  # noqa: F401
from .train import FusedTrainer, PlateauLR  # noqa: F401
from .metrics import (GroupMetrics, ListMetrics, Metrics, eval_metrics, evaluate,  # noqa: F401
                      evaluate_ranking, group_metrics, list_metrics, list_metrics_raw,
                      popularity_information, roc_auc_score)
from . import serving  # noqa: F401
from .data import DeviceLoader  # noqa: F401
from .serving import RankingPipeline, rerank_with_mmr  # noqa: F401
from .interactions import InteractionStore  # noqa: F401
from .cities import CitySets  # noqa: F401
from .item_features import ItemFeatures  # noqa: F401
from .prepare import PreparedData, category_keys, prepare_data, prepare_data_host  # noqa: F401
from .transform import IdMap, Preprocessor, Transformed  # noqa: F401
from . import artifacts  # noqa: F401

__version__ = "0.1.0"
