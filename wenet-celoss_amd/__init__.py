"""MI355X-native CTC / RNN-T loss and transducer decode for WeNet.

Host side: thin PyTorch shims that mirror the reference's call sites
(wenet/transducer/transducer.py, wenet/transformer/ctc.py, wenet/transducer/
joint.py, wenet/transducer/search/*.py) and forward device pointers to
libwr_mi355x.so (include/wr_api.h).  There is no CPU fallback.
"""
from . import _lib  # noqa: F401
from .rnnt_loss import rnnt_loss, RNNTLoss  # noqa: F401
from .ctc import CTC, ctc_loss, ctc_greedy_search, ctc_prefix_beam_search, forced_align, forced_align_batch  # noqa: F401
from .ctc import CtcPrefixBeamStream, ctc_prefix_beam_search_times  # noqa: F401
from .ctc import CtcContextPrefixBeamStream, ctc_context_prefix_beam_search  # noqa: F401
from .context_graph import ContextGraph  # noqa: F401
from .joint import TransducerJoint, joint_logits  # noqa: F401
from .fused import joint_rnnt_loss, joint_rnnt_tdt_loss  # noqa: F401
from .rnnt_align import joint_rnnt_forced_align, rnnt_forced_align, rnnt_frame_tokens  # noqa: F401
from .rnnt_simple import rnnt_loss_simple, rnnt_simple_forced_align  # noqa: F401
from .rnnt_smoothed import rnnt_loss_smoothed  # noqa: F401
from .rnnt_pruned import do_rnnt_pruning, get_rnnt_prune_ranges, rnnt_loss_pruned  # noqa: F401
from .rnnt_tdt import TDTLoss, rnnt_tdt_forced_align, rnnt_tdt_lattice, rnnt_tdt_loss  # noqa: F401
from .predictor import ConvPredictor, EmbeddingPredictor, PredictorBase, RNNPredictor  # noqa: F401
from .search.greedy_search import (basic_greedy_search, basic_greedy_search_both,  # noqa: F401
                                   basic_greedy_search_hw, edit_distance, tdt_greedy_search)
from .search.prefix_beam_search import (PrefixBeamSearch, Sequence, TransducerContextPrefixBeamStream,  # noqa: F401
                                        TransducerPrefixBeamStream, tdt_prefix_beam_search)
from . import k2  # noqa: F401  (the k2 functions with k2's signatures: rnnt_type=, delay_penalty=)
from .transducer import Transducer  # noqa: F401
from .common import IGNORE_ID, add_blank, log_add  # noqa: F401

__all__ = ["rnnt_loss", "RNNTLoss", "CTC", "ctc_loss", "TransducerJoint", "joint_logits", "joint_rnnt_loss", "RNNPredictor",
           "EmbeddingPredictor", "ConvPredictor", "PredictorBase",
           "basic_greedy_search", "PrefixBeamSearch", "Sequence", "Transducer", "IGNORE_ID", "add_blank", "log_add",
           "ctc_greedy_search", "ctc_prefix_beam_search", "forced_align", "forced_align_batch", "rnnt_forced_align",
           "joint_rnnt_forced_align", "rnnt_frame_tokens", "rnnt_loss_simple", "rnnt_simple_forced_align", "rnnt_loss_smoothed",
           "get_rnnt_prune_ranges", "do_rnnt_pruning", "rnnt_loss_pruned", "k2",
           "rnnt_tdt_loss", "TDTLoss", "rnnt_tdt_lattice", "joint_rnnt_tdt_loss", "tdt_greedy_search", "rnnt_tdt_forced_align",
           "tdt_prefix_beam_search", "CtcPrefixBeamStream", "ctc_prefix_beam_search_times",
           "ContextGraph", "CtcContextPrefixBeamStream", "ctc_context_prefix_beam_search", "TransducerPrefixBeamStream",
           "TransducerContextPrefixBeamStream"]
