"""skge_amd -- MI355X-native (HIP/gfx950) scikit-kge training hot path.

Drop-in for skge's model / updater / trainer protocol: TransE, HolE, RESCAL,
DistMult, ComplEx, RotatE, StochasticTrainer, PairwiseStochasticTrainer, SGD, AdaGrad,
RandomModeSampler, CorruptedSampler, LCWASampler.  Every numeric step runs in libskgehip.so."""
from .version import __version__
from .base import (Model, StochasticTrainer, PairwiseStochasticTrainer, SelfAdversarialTrainer,
                   set_deterministic, deterministic)
from .kvsall import KvsAllTrainer, KvsAllQueries
from .onevsall import OneVsAllTrainer, OneVsAllQueries
from .transe import TransE
from .hole import HolE
from .rescal import RESCAL
from .distmult import DistMult
from .complex import ComplEx
from .rotate import RotatE
from .param import Parameter, SGD, AdaGrad, normalize, normless1, unitmod
from .sample import RandomModeSampler, CorruptedSampler, LCWASampler, type_index
from .eval import (FilteredRankingEval, TransEEval, HolEEval, compute_scores, ranking_scores,
                   relation_ranking_scores, pool_csr, type_pools)
from .predict import LinkPredictor
from .subgraphs import SUBTYPE, Subgraphs, SubgraphRankingEval, subgraph_ranking_scores
from .neighbours import Neighbours, shared_role
from .linkpred import (LinkPredictionEval, TripleClassifier, link_prediction_callback,
                       score_triples, curve_stats)
from .checkpoint import save_reference, load_reference, read_reference_state
