"""The reference's own model classes as the golden writers build them: no backbone, everything else untouched.  Imports the READ-ONLY
reference checkout through oracle._ref_import, so only oracle/make_golden_*.py import this module -- never a test, smoke() or bench.py."""
import torch

from oracle import _ref_import

_ref_import.setup()
from models.DCMHT.DCMHT import DCMHT  # noqa: E402  (the reference classes)
from models.DCMHT.hash.hash import HashLayer as DCMHTHashLayer  # noqa: E402,F401
from models.DSPH.DSPH import DSPH  # noqa: E402
from models.DSPH.hash.hash import HashLayer as DSPHHashLayer  # noqa: E402,F401
from models.MITH.MITH import MITH  # noqa: E402


def dcmht(K, sim="euclidean", vartheta=0.75, threshold=0.1, quan_alpha=0.001):
    m = DCMHT.__new__(DCMHT)                       # the loss methods only read these attributes; no backbone is built
    torch.nn.Module.__init__(m)
    m.output_dim, m.vartheta, m.threshold, m.similarity_function, m.quan_alpha = K, vartheta, threshold, sim, quan_alpha
    return m


def _no_backbone(cls, width):
    return type("NoBackbone", (cls,), {"load_backbone": lambda self, clipPath, return_patches=False: (width, torch.nn.Identity())})


def dsph(K, C, alpha, width=8, hypseed=0):
    """built by the reference's own DSPH.__init__, so its HyP threshold is the codetable cell the reference looks up for (K, C)"""
    return _no_backbone(DSPH, width)(cfg=None, outputDim=K, numclass=C, hypseed=hypseed, alpha=alpha)


def mith(N, K, D, weights):
    return _no_backbone(MITH, D)(cfg=None, outputDim=K, train_num=N, **weights)
