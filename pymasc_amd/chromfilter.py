"""Chromosome include / exclude filters: PyMaSC's ``-i/--include-chrom`` and ``-e/--exclude-chrom`` (utils/parsearg.py,
the filter itself in utils/calc.py ``filter_chroms``, applied to the BAM header in reader/bam.py ``apply_chromfilter``).

A filter is an ordered list of groups ``(include, patterns)``, one per option on the command line.  Consecutive groups of the
same kind act as one.  The patterns are ``fnmatch`` patterns (case-sensitive).  Walking the groups in order with a current
set that starts as every reference:

* an include group narrows the current set to the names that match;
* an exclude group keeps the current names that do not match, and the current set becomes the names that do match, so that
  a following include group can take some of them back;
* after the last group, the current set is kept as well when that group was an include group.

The result is in header order.  A filter that leaves nothing raises ``NoTargetChromosomesError`` (PyMaSC's
BAMNoTargetChroms).
"""
from __future__ import annotations

import fnmatch
from typing import List, Optional, Sequence, Tuple

ChromFilter = Sequence[Tuple[bool, Sequence[str]]]


class NoTargetChromosomesError(ValueError):
    """The chromosome filter leaves no reference of the BAM header."""


def _merged(chromfilter: ChromFilter) -> List[Tuple[bool, List[str]]]:
    groups: List[Tuple[bool, List[str]]] = []
    for include, patterns in chromfilter:
        if isinstance(patterns, str):
            patterns = [patterns]
        if groups and groups[-1][0] == bool(include):
            groups[-1][1].extend(patterns)
        else:
            groups.append((bool(include), list(patterns)))
    return groups


def filter_references(references: Sequence[str], chromfilter: Optional[ChromFilter]) -> List[str]:
    """The names of ``references`` (header order) that ``chromfilter`` keeps; None or an empty filter keeps all of them."""
    if not chromfilter:
        return list(references)
    current = set(references)
    kept = set()
    include = True
    for include, patterns in _merged(chromfilter):
        matched = {n for n in current if any(fnmatch.fnmatchcase(n, p) for p in patterns)}
        if not include:
            kept |= current - matched
        current = matched
    if include:
        kept |= current
    out = [n for n in references if n in kept]
    if not out:
        raise NoTargetChromosomesError("the chromosome filter {!r} leaves no reference of the BAM file".format(list(chromfilter)))
    return out


def kept_references(header: Sequence[str], references: Optional[Sequence[str]], chromfilter: Optional[ChromFilter]) -> List[str]:
    """The names of a reader's ``header`` that a run keeps, in header order: what ``chromfilter`` leaves when one is given, else
    the ones named in ``references`` (None: all of them)."""
    if chromfilter is not None:
        return filter_references(header, chromfilter)
    return [n for n in header if references is None or n in set(references)]
