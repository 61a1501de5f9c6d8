"""A/B rounds of a timing script (the scripts that take --ab LABEL: the simulated-quantum-annealing ones and those of the
replica measurements and moves): one
run times one library -- the tree's, or the one SGA_LIBRARY_PATH names -- and appends its figures as a round under
doc["ab_rounds"][LABEL][cell]; two libraries alternate in one session by alternating runs.  Nothing else of the file is
touched.  doc["ab_rounds"]["summary"][cell][figure][LABEL] is rewritten with every round: the median of the rounds'
medians and their spread [min, max] -- a difference between two labels is held against the round-to-round spread of each."""
import numpy as np


def append(doc, label, cell, figures, library):
    """figures: name -> [median, min, max] ms of one run"""
    ab = doc.setdefault("ab_rounds", {})
    ab.setdefault(label, {}).setdefault(cell, []).append(dict(figures, library=library))
    summary = {}
    for lab, cells in ab.items():
        if lab == "summary":
            continue
        for c, rounds in cells.items():
            for name in rounds[0]:
                if name == "library":
                    continue
                medians = [r[name][0] for r in rounds]
                summary.setdefault(c, {}).setdefault(name, {})[lab] = {
                    "median_of_rounds": float(np.median(medians)), "spread": [min(medians), max(medians)], "rounds": len(medians)}
    ab["summary"] = summary
