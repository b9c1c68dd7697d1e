"""The stages of the reference's annotation.py that work on Guide objects: reverse_guides (annotation.py:27-51), which the
scorers depend on, and ann_guides (annotation.py:465-510), the BED / gene annotation of a guide list - one device join per
file (bedannot.AnnotTable) instead of one tabix fetch per guide.  Variant polishing and GC content are computed per report
group in reports.py."""
from typing import List, Union

import numpy as np

from .guide import Guide
from .utils import VERBOSITYLVL, print_verbosity


def reverse_guides(guides: List[Guide], verbosity: int) -> List[Guide]:
    print_verbosity("Reversing guides occurring on reverse strand", verbosity, VERBOSITYLVL[3])
    for guide in guides:
        if guide.strand == 1:
            guide.reverse_complement()
    return guides


def ann_guides(guides: List[Guide], contig: str, annotations: List[Union[str, "BedAnnotation"]], atype: int, verbosity: int,
               debug: bool) -> List[Guide]:
    """annotation.py:465-510, same arguments: every guide gets one entry per file appended to `funcann` (atype 0: the 4th BED
    column of the overlapping features) or `geneann` (atype 1: feature:gene_name), "NA" without an overlap or for a contig the
    file does not have.  `annotations` holds paths or opened bedannot.BedAnnotation objects (a path is opened and closed here)."""
    from .bedannot import BedAnnotation
    print_verbosity("Starting guides annotation", verbosity, VERBOSITYLVL[3])
    assert atype in {0, 1}
    starts = np.array([g.start for g in guides], dtype=np.int64)
    stops = np.array([g.stop for g in guides], dtype=np.int64)
    for fann in annotations:
        bedann = fann if isinstance(fann, BedAnnotation) else BedAnnotation(fann, verbosity, debug)
        try:
            labels = bedann.table(contig, atype).query(starts, stops).strings()
        finally:
            if bedann is not fann:
                bedann.close()
        for guide, label in zip(guides, labels):
            if atype == 0:
                guide.funcann = label
            else:
                guide.geneann = label
    return guides
