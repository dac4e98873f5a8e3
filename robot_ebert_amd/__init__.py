"""robot_ebert_amd -- MI355X-native embedding-similarity retrieval for robot-ebert's recommend path.

The hot path (query x catalog cosine + top-k, reference src/backend/app/lib.py:51-55) runs in
hand-written HIP kernels for gfx950 behind the C ABI of include/ebert.h (libebert.so, loaded by
ctypes). Python keeps the reference's call surface: ``lib.get_user_recs`` and friends.

The resident ``Catalog`` is live: ``Catalog.update_rows`` / ``Catalog.append`` (ABI 0.4.0) replace
and append rows in place, and ``Catalog.remove`` (ABI 0.5.0) removes rows in place, filling the
holes from the tail and returning the moves ``(old_row, new_row)``; ``RecBatcher.update_rows`` /
``.append`` / ``.remove`` do so between batches and ``distributed.split_update`` hands each shard
of a row-sharded catalog its part of an update.

``AllowMasks`` (ABI 0.6.0) restricts a query to a subset of the rows: ``score_topk(..., allow=(masks,
mask_ids))`` returns the top k of (allowed rows minus excluded rows). A sparse mask can be
materialised (ABI 0.7.0): ``masks.materialize(mask)`` copies its allowed rows into a dense
sub-catalog (``SubCatalog``) and the queries of that mask are then scored over those rows alone,
with the same rows and bitwise the same scores.

Liked rows can carry weights (ABI 0.8.0): ``score_topk(..., liked=, liked_weights=)`` scores by
sum_l w_l cos(x_l, x) / sum_l |w_l| (negative weights push away), through every path the
unweighted call has; ``lib.get_user_recs(..., weighting=)`` maps a user's ratings to weights.

``explain_topk`` (ABI 0.9.0) says why: for the rows a search returned, the per-liked-row terms of
each score and the m largest of them; ``lib.get_user_recs_explained`` attaches them as reasons.

``diversify_topk`` (ABI 0.10.0) trades relevance for variety: from a pool of the p best rows it
picks k greedily by maximal marginal relevance, lam * score - (1 - lam) * (largest cosine to a
row already picked); ``lib.get_user_recs_diverse`` is the recommend call over it.

``multi_interest_topk`` (ABI 0.11.0) serves a user with several tastes: ``cluster_liked`` groups
the liked rows into up to c clusters, each cluster is searched on its own, and the answers are
interleaved in proportion to the clusters' sizes; ``lib.get_user_recs_interests`` is the recommend
call over it ("more like X", X the cluster's medoid).

``score_topk_grouped`` (ABI 0.12.0) fills a front page: the top k of every query within each of G
allow masks ("top drama for you", "top comedy for you") from ONE scoring pass, each shelf bit for
bit what ``score_topk(..., allow=)`` returns for that mask; ``lib.get_user_recs_by_group`` is the
recommend call over it.
"""
from ._lib import EbertError, Timer, load  # noqa: F401
from .catalog import Catalog  # noqa: F401
from .allow import AllowMasks, SubCatalog  # noqa: F401
from .search import (merge_topk, prepare_queries, rescore_rows, score_topk,  # noqa: F401
                     score_topk_finish, score_topk_submit)
from .explain import Explanation, explain_topk  # noqa: F401
from .diversify import Diversified, diversify_topk  # noqa: F401
from .interests import (Interests, MultiInterest, cluster_liked,  # noqa: F401
                        multi_interest_topk)
from .grouped import GroupedTopk, score_topk_grouped  # noqa: F401
from . import ops  # noqa: F401,E402  (registers torch.ops.ebert.*)

__version__ = "0.1.0"
