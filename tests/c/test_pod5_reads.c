/* The reads-table reader of include/pgnano_pod5file.h from plain C, host only: built together with
 * csrc/pgn_pod5file.cpp (no GPU code, no HIP runtime), so it can run under the host sanitizers:
 *   g++ -fsanitize=address,undefined -c pgn_pod5file.cpp; gcc -fsanitize=... -c test_pod5_reads.c; g++ link
 *   test_pod5_reads <file.pod5> <scratch path>
 * Opens the file, reads its reads table with every array and with none, then writes copies of the
 * file cut short or with bytes of the reads table overwritten and reads those: each must give a
 * status, never a fault. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pgnano_pod5file.h"

#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                \
        }                                                            \
    } while (0)

static int write_all(const char *path, const unsigned char *p, size_t n)
{
    FILE *fp = fopen(path, "wb");
    if (!fp) return 1;
    const size_t w = fwrite(p, 1, n, fp);
    return fclose(fp) != 0 || w != n;
}

/* reads the table of `path` with exactly sized arrays; returns the status of open or of the read */
static int read_table(const char *path, uint64_t *reads_out)
{
    pgn_pod5_file *f = NULL;
    int rc = pgn_pod5_file_open(path, &f);
    if (rc) return rc;
    uint64_t reads = 0, entries = 0;
    uint32_t batches = 0;
    rc = pgn_pod5_reads_info(f, &reads, &batches, &entries);
    if (rc == PGN_OK) {
        uint8_t *ids = malloc(16 * reads + 1), *well = malloc(reads + 1);
        uint64_t *first = malloc(8 * (reads + 1)), *rows = malloc(8 * entries + 1), *ns = malloc(8 * reads + 1),
                 *ss = malloc(8 * reads + 1);
        float *off = malloc(4 * reads + 1), *scale = malloc(4 * reads + 1);
        uint32_t *num = malloc(4 * reads + 1);
        uint16_t *ch = malloc(2 * reads + 1);
        rc = pgn_pod5_reads_read(f, ids, first, rows, ns, ss, off, scale, num, ch, well);
        if (rc == PGN_OK) {
            uint64_t rowsTotal = 0;
            pgn_pod5_signal_info(f, &rowsTotal, NULL, NULL, NULL, NULL);
            if (first[0] != 0 || first[reads] != entries) rc = -1;
            for (uint64_t r = 0; r < reads && rc == PGN_OK; r++)
                if (first[r + 1] < first[r]) rc = -1;
            for (uint64_t k = 0; k < entries && rc == PGN_OK; k++)
                if (rows[k] >= rowsTotal) rc = -1;
        }
        if (rc == PGN_OK) rc = pgn_pod5_reads_read(f, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
        free(ids); free(well); free(first); free(rows); free(ns); free(ss); free(off); free(scale); free(num); free(ch);
        if (reads_out) *reads_out = reads;
    }
    pgn_pod5_file_close(f);
    return rc;
}

int main(int argc, char **argv)
{
    if (argc < 3) {
        fprintf(stderr, "usage: %s file.pod5 scratch-path\n", argv[0]);
        return 2;
    }
    uint64_t reads = 0;
    CHECK(read_table(argv[1], &reads) == PGN_OK);
    CHECK(reads > 0);
    CHECK(pgn_pod5_reads_info(NULL, NULL, NULL, NULL) == PGN_ERR_INVALID_ARG);

    /* the file image and where its reads table sits */
    FILE *fp = fopen(argv[1], "rb");
    CHECK(fp);
    CHECK(fseek(fp, 0, SEEK_END) == 0);
    const long size = ftell(fp);
    CHECK(size > 0);
    rewind(fp);
    unsigned char *img = malloc((size_t)size), *work = malloc((size_t)size);
    CHECK(img && work && fread(img, 1, (size_t)size, fp) == (size_t)size);
    fclose(fp);
    pgn_pod5_file *f = NULL;
    CHECK(pgn_pod5_file_open(argv[1], &f) == PGN_OK);
    int64_t off = -1, len = 0;
    for (int i = 0; i < pgn_pod5_file_embedded_count(f); i++) {
        int64_t o, l;
        int type;
        CHECK(pgn_pod5_file_embedded(f, i, &o, &l, &type) == PGN_OK);
        if (type == PGN_POD5_CONTENT_READS) {
            off = o;
            len = l;
        }
    }
    pgn_pod5_file_close(f);
    CHECK(off > 0 && len > 0 && off + len <= size);

    /* cut short: the end of the file is gone, the open itself must refuse */
    int statuses = 0;
    for (int k = 1; k <= 4; k++) {
        CHECK(write_all(argv[2], img, (size_t)size * k / 5) == 0);
        CHECK(read_table(argv[2], NULL) != PGN_OK);
        statuses++;
    }
    /* stretches of 1 to 8 bytes of the reads table overwritten, anywhere from its schema to its footer */
    unsigned seed = 12345u;
    for (int k = 0; k < 200; k++) {
        memcpy(work, img, (size_t)size);
        seed = seed * 1664525u + 1013904223u;
        const int64_t at = off + (int64_t)((seed >> 8) % (uint64_t)len);
        seed = seed * 1664525u + 1013904223u;
        int64_t n = 1 + (seed >> 16) % 8;
        if (at + n > off + len) n = off + len - at;
        for (int64_t i = 0; i < n; i++) {
            seed = seed * 1664525u + 1013904223u;
            work[at + i] = (unsigned char)(seed >> 24);
        }
        CHECK(write_all(argv[2], work, (size_t)size) == 0);
        const int rc = read_table(argv[2], NULL);
        CHECK(rc >= 0); /* -1: a successful parse gave inconsistent arrays */
        if (rc != PGN_OK) statuses++;
    }
    /* the whole table zeroed from its middle on */
    memcpy(work, img, (size_t)size);
    memset(work + off + len / 2, 0, (size_t)(len - len / 2));
    CHECK(write_all(argv[2], work, (size_t)size) == 0);
    CHECK(read_table(argv[2], NULL) != PGN_OK);
    remove(argv[2]);
    free(img);
    free(work);
    printf("test_pod5_reads ok: %llu reads, %d damaged copies refused\n", (unsigned long long)reads, statuses);
    return 0;
}
