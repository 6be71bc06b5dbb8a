#!/usr/bin/env python3
"""Kernel statistics split by launch shape (name, grid size) from a rocprofv3 rocpd SQLite file: the multigrid
kernels run once per level with a grid of their own, so the grid names the level.
    tools/rocpd_by_grid.py results.db out.csv [name-substring ...]"""
import csv
import sqlite3
import sys

db = sqlite3.connect(sys.argv[1])
subs = sys.argv[3:] or [""]
where = " or ".join("name like ?" for _ in subs)
rows = db.execute(f"select name, grid_x, count(*), avg(end-start), min(end-start), max(end-start) from kernels where {where} "
                  "group by name, grid_x order by name, grid_x desc", [f"%{x}%" for x in subs]).fetchall()
with open(sys.argv[2], "w", newline="") as f:
    w = csv.writer(f)
    w.writerow(["Name", "GridX", "Calls", "AverageNs", "MinNs", "MaxNs"])
    for r in rows:
        w.writerow([r[0], r[1], r[2], round(r[3], 1), r[4], r[5]])
for r in rows:
    print(r[0][:48].ljust(48), str(r[1]).rjust(9), str(r[2]).rjust(6), f"{r[3] / 1e3:8.2f} us")
