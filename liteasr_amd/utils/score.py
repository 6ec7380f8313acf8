"""Scoring (liteasr/utils/score.py)."""


def levenshtein(a, b):
    """Edit distance between two sequences (strings, lists, tuples): unit cost for an insertion,
    a deletion and a substitution.  One row of the table is kept, over the shorter sequence."""
    if len(a) > len(b):
        a, b = b, a
    row = list(range(len(a) + 1))
    for i, bi in enumerate(b, 1):
        diag, row[0] = row[0], i
        for j, aj in enumerate(a, 1):
            diag, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, diag + (aj != bi))
    return row[len(a)]
