// options.h -- the row that states one process-wide switch (r3g_set_option / r3g_get_option; internal to libr3g.so).
// A file that owns switches keeps its variables as plain ints beside the code that reads them and, under them, ONE array of rows that
// ends in an empty row {}; model.cpp walks the arrays.  A new switch is a variable, a row, the prose in include/r3g.h and a row in
// tests/switch_table.py.
#ifndef R3G_OPTIONS_H
#define R3G_OPTIONS_H

namespace r3g {

// what a set does with its value; `ok` says which values a row takes as they are
enum OptionRule {
    OPT_FLAG,     // stored as value != 0
    OPT_ANY,      // any integer
    OPT_KEEP,     // !ok(value): ignored -- the old value stays and the call still returns R3G_OK
    OPT_ELSE,     // !ok(value): `other` is stored instead
    OPT_MASK,     // value & other
    OPT_REFUSE,   // !ok(value): R3G_ERR_INVALID with `refusal`, the old value stays
};

struct Option {
    const char* name = nullptr;      // null: the end of the array
    int* slot = nullptr;             // the variable; r3g_get_option reports it as it is
    OptionRule rule = OPT_FLAG;
    bool (*ok)(int) = nullptr;
    int other = 0;
    const char* refusal = nullptr;
    bool new_epoch = true;           // a set starts a new option epoch: results cached under the old value are built again (model.cpp)
    int* slot2 = nullptr;            // "lds_dma" alone: a second variable that a set writes as well; a get reports 1 while both are
};

// what r3g_set_option does with a known name apart from the new epoch (r3g_create sets "gemm_num_cu" this way); unknown name: R3G_ERR_INVALID
int option_store(const char* name, int value);

}  // namespace r3g
#endif
